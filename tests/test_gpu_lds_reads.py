"""GPU parity of the fp32 n = 16384 one-pass kernels with their 8-byte LDS reads issued from
inline asm (NW_LDS_ASM_READS, nw_shape.h: the 1 -> 2 image's pairs and the pass-1 twiddle table).

Morse scales 2, 60, 120, 170, 200, 230, 256, 320 and 450 Hz at 1 kHz run all seven pass-0 variants
(asserted with tests/fused_variants.py), whose pruned outputs feed the table's twiddles.  With
9 signals and 9 scales the output kernels run blocks of 2, 2, 2, 2 and 1 signals (group_filling,
nw_shape.h, halves the block of a launch this small: the loop-carried DMA and its counted wait
over one signal boundary), 2 signals a block of two; only the partial-sum kernel behind power_mean
keeps a block of 8 and a block of one.  Blocks of 8 of the output kernels:
tests/test_gpu_fused_rows.py, tests/test_gpu_chunk_parity.py.  cwt, |y|, |y|^2 and power_mean against oracle.nw_oracle at the bounds of
tests/test_gpu_parity.py (1e-5 of max; 2e-5 for |y|^2 and power_mean).

A complex-table-row wavelet (the `paul` plugin of tests/plugins.py; 3 scales x 3 signals, cwt and
|y|^2) takes the image and table reads without the X DMA.  Interleaved: plan A (Morse), then the
table-row wavelet, then A again -- A's two outputs are bitwise equal: no read leaves a stale
batch in registers or in the table."""
import numpy as np
import pytest

import plugins
from fused_variants import instantiated_variants, row_wnz, variant_of
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

N, S, SFREQ, DTYPE = 16384, 9, 1000., 'float32'
FREQS = np.array([2., 60., 120., 170., 200., 230., 256., 320., 450.])
PAUL_FREQS = [3., 10., 40.]
TOL = 1e-5

_cache = {}


def signals():
    if 'x' not in _cache:
        rng = np.random.default_rng(15)
        t = np.arange(N) / SFREQ
        fc = rng.uniform(2, 300, (S, 1))
        x = np.sin(2 * np.pi * fc * t + rng.uniform(0, 6.28, (S, 1))) + 0.2 * rng.standard_normal((S, N))
        _cache['x'] = x.astype(DTYPE)
        _cache['x'].setflags(write=False)
    return _cache['x']


def reference():
    """The oracle's complex CWT of every signal, (S, F, N) complex128, computed once."""
    if 'ref' not in _cache:
        _cache['ref'] = np.stack([O.cwt('morse', xi.astype(np.float64), FREQS) for xi in signals()])
        _cache['ref'].setflags(write=False)
    return _cache['ref']


def paul():
    return plugins.make(nw, 'paul', SFREQ, False, dtype=DTYPE)


def paul_reference():
    """(3, 3, N) complex128: the oracle's plugin CWT of the first three signals."""
    if 'paul' not in _cache:
        w = paul()
        _cache['paul'] = np.stack([O.plugin_cwt(w.mode.name, w.trans_formula, w.formula, w.peak_freq,
                                                xi.astype(np.float64), PAUL_FREQS, sfreq=SFREQ)[0] for xi in signals()[:3]])
        _cache['paul'].setflags(write=False)
    return _cache['paul']


def of_kind(ref, out):
    return ref if out == 'cwt' else np.abs(ref) if out == 'abs' else np.abs(ref) ** 2


def check(got, want, tol, what):
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f'{what}: rel err {err:.3e} (tol {tol:.0e})')
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= tol * np.max(np.abs(want)) + 1e-30, (what, err)


def plan(max_batch=S):
    p = nw.Plan(N, len(FREQS), DTYPE, max_batch=max_batch)
    p.set_wavelet('morse', [17.5, 3.0], FREQS.astype(np.float64), L.trans_grid(N / SFREQ, SFREQ, False))
    return p


def test_scales_run_every_pass0_variant():
    p = plan()
    try:
        rows = p.rows()
    finally:
        p.close()
    for out in ('cwt', 'abs', 'power'):
        variants = instantiated_variants(N, DTYPE, out, False)
        hit = [variant_of(row_wnz(r, N, DTYPE)[0], variants) for r in rows]
        print(f'{out}: variants {hit}')
        assert variants == {4, 8, 12, 16, 20, 24, 32}
        assert set(hit) == variants, (out, hit)


@pytest.mark.parametrize('nsig', [9, 2])
@pytest.mark.parametrize('out', ['cwt', 'abs', 'power'])
def test_signals_against_oracle(out, nsig):
    p = plan(max_batch=nsig)
    try:
        got = p.execute(signals()[:nsig], out_kind=out)
        st = p.stats()
    finally:
        p.close()
    assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_kernel', st
    check(got, of_kind(reference()[:nsig], out), TOL * (2 if out == 'power' else 1), f'{nsig} signals {out}')


@pytest.mark.parametrize('nsig', [9, 2])
def test_power_mean(nsig):
    p = plan(max_batch=nsig)
    try:
        pm = p.execute(signals()[:nsig], out_kind='power_mean')
    finally:
        p.close()
    check(pm, np.mean(np.abs(reference()[:nsig]) ** 2, axis=0), 2e-5, f'power_mean of {nsig}')


@pytest.mark.parametrize('out', ['cwt', 'power'])
def test_complex_table_rows(out):
    got = paul().cwt_batch(signals()[:3], PAUL_FREQS, out=out)
    check(got, of_kind(paul_reference(), out), TOL * (2 if out == 'power' else 1), f'paul {out}')


@pytest.mark.parametrize('out', ['cwt', 'power'])
def test_interleaved_plans_repeat_bitwise(out):
    w = paul()
    p = plan()
    try:
        a1 = p.execute(signals(), out_kind=out)
        b = w.cwt_batch(signals()[:3], PAUL_FREQS, out=out)
        a2 = p.execute(signals(), out_kind=out)
    finally:
        p.close()
    check(b, of_kind(paul_reference(), out), TOL * (2 if out == 'power' else 1), f'paul between {out}')
    check(a1, of_kind(reference(), out), TOL * (2 if out == 'power' else 1), f'A first {out}')
    assert np.array_equal(a1.view(np.uint8), a2.view(np.uint8)), 'plan A differs after plan B ran'
