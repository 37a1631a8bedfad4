"""-DNW_DFT_DIF still builds (CPU: device-only compiles, nothing runs).

The switch selects the radix-2 DIF register DFTs with separate twiddle multiplies (the
arithmetic up to round 6, nw_dft_reg.h) in every user of the templates; tools/ab.sh measures
the FMA form against a library built with it (make VARIANT=dif DEFS=-DNW_DFT_DIF), so it has
to keep compiling, as the switches of tests/test_diag_builds.py do."""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = '/opt/rocm/bin/hipcc'
CSRC = os.path.join(ROOT, 'ninwavelets_amd', 'csrc')
SOURCES = ['nw_fused.hip', 'nw_large.hip', 'nw_chirp.hip']


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_dif_form_compiles(tmp_path):
    procs = [(src, subprocess.Popen(
        [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++20', '-fno-slp-vectorize', '--cuda-device-only',
         '-DNW_DFT_DIF', '-c', os.path.join(CSRC, src), '-o', str(tmp_path / (src + '.co'))],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for src in SOURCES]
    for src, p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, f'{src}: {err[-2000:]}'
        assert os.path.getsize(tmp_path / (src + '.co')) > 0
