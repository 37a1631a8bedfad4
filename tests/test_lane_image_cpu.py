"""The lane-addressed exchange images of the fp32 n = 16384 kernels, checked without a GPU.

tests/host/lane_image_check.cpp includes ninwavelets_amd/csrc/nw_shape.h (namespace lane_image,
the functions the kernels compile) and checks, for every thread, slot and component of both images:
  1. writer and reader addresses against the padded images' slot formulas (a bijection);
  2. every wave store is base + 4 * lane from a wave-uniform base (ds_write_addtid_b32);
  3. ds_read_b32 groups conflict-free over 32 banks in 32-lane groups;
  4. ds_read_b64 groups conflict-free over 64 banks in 32-lane groups;
  5. offsets and M0 below 65536 (their 16-bit fields) and M0 + offset + 252, the last lane's
     dword, inside the image (max 65656 for the 0 -> 1 and 69500 for the 1 -> 2 image, of
     69632 B: with the row strides 513 and 544 the sum cannot stay below 65536 as well);
  6. twice (image + pass-1 table) within the CU's 160 KiB.
It is built with -fsanitize=address,undefined and run as a stand-alone program.

The old layout stays behind -DNW_LANE_IMAGE=0: that build of nw_fused.hip compiles (device
only, nothing runs) and holds none of the new stores."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')


def test_lane_image_layout_under_asan(tmp_path):
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'lane_image_check')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'lane_image_check.cpp'),
                    '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'ok'
    fig = dict(zip(lines[0].split()[::2], map(int, lines[0].split()[1::2])))
    assert fig['max_offset'] < 65536 and fig['max_m0'] < 65536
    assert fig['max_m0_offset_252'] + 4 <= fig['image_bytes'] == 32 * 544 * 4
    assert fig['lds_two_blocks'] <= 160 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_old_layout_switch_compiles(tmp_path):
    out = tmp_path / 'nw_fused_old.s'
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++20', '-fno-slp-vectorize', '--cuda-device-only',
                        '-DNW_LANE_IMAGE=0', '-S', os.path.join(ROOT, 'ninwavelets_amd', 'csrc', 'nw_fused.hip'),
                        '-o', str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    assert 'nw_fused_kernel' in text and 'ds_write_addtid_b32' not in text
