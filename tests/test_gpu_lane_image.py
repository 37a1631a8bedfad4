"""GPU parity of the fp32 n = 16384 one-pass kernels, whose two LDS exchanges run on the
lane-addressed images (nw_shape.h, lane_image; ds_write_addtid_b32 stores).

fp32, n = 16384, 9 signals and 9 scales: the output kernels run blocks of 2, 2, 2, 2 and 1 signals
(group_filling, nw_shape.h, halves the block of a launch this small; the next signal's X by LDS-DMA
into the image region over one signal boundary), the partial-sum kernel behind power_mean a block
of 8 and a block of one.  Blocks of 8 of the output kernels: tests/test_gpu_fused_rows.py,
tests/test_gpu_chunk_parity.py.  Morse scales 2, 60, 120, 170, 200, 230, 256 Hz at
1 kHz run the pass-0 variants 4, 8, 12, 16 and 20; 320 and 450 Hz add 24 and 32 (rows that read
mirrored bins), so all seven variants of the kernel run.  Which variant a row runs is read off the
plan's own W rows by the rule of tests/fused_variants.py (compared with nw_shape.h by
tests/test_host_asan.py; nw_plan_row_support serves two-pass plans only), and the set is asserted.

Outputs cwt, |y| and |y|^2 against oracle.nw_oracle at the bounds of tests/test_gpu_parity.py
(1e-5 of max, 2e-5 for |y|^2), the same at one scale and one signal, the power-mean and ITC
reductions at that file's bounds (2e-5 of max; ITC 2e-5 where every epoch's |cwt| >= 0.1 of its
row's max and 1e-3 everywhere), and one decimated call (exactly cwt[..., ::4], 1e-5 of max)."""
import numpy as np
import pytest

from fused_variants import instantiated_variants, row_wnz, variant_of
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

N, S, SFREQ, DTYPE = 16384, 9, 1000., 'float32'
FREQS = np.array([2., 60., 120., 170., 200., 230., 256., 320., 450.])
TOL = 1e-5

_cache = {}


def signals():
    if 'x' not in _cache:
        rng = np.random.default_rng(16384)
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


def of_kind(ref, out):
    return ref if out == 'cwt' else np.abs(ref) if out == 'abs' else np.abs(ref) ** 2


def check(got, want, tol, what):
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f'{what}: rel err {err:.3e} (tol {tol:.0e})')
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= tol * np.max(np.abs(want)) + 1e-30, (what, err)


def plan(freqs, max_batch=S, **kw):
    p = nw.Plan(N, len(freqs), DTYPE, max_batch=max_batch, **kw)
    p.set_wavelet('morse', [17.5, 3.0], np.asarray(freqs, dtype=np.float64), L.trans_grid(N / SFREQ, SFREQ, False))
    return p


def test_scales_run_every_pass0_variant():
    p = plan(FREQS)
    try:
        rows = p.rows()
    finally:
        p.close()
    assert rows.shape == (len(FREQS), N)
    for out in ('cwt', 'abs', 'power'):
        variants = instantiated_variants(N, DTYPE, out, False)
        hit = [variant_of(row_wnz(r, N, DTYPE)[0], variants) for r in rows]
        print(f'{out}: variants {hit}')
        assert variants == {4, 8, 12, 16, 20, 24, 32}
        assert set(hit) == variants, (out, hit)


@pytest.mark.parametrize('out', ['cwt', 'abs', 'power'])
def test_nine_signals_against_oracle(out):
    got = nw.Morse(SFREQ, dtype=DTYPE).cwt_batch(signals(), FREQS, out=out)
    check(got, of_kind(reference(), out), TOL * (2 if out == 'power' else 1), f'9 signals {out}')


@pytest.mark.parametrize('out', ['cwt', 'abs', 'power'])
def test_one_scale_one_signal(out):
    k = 2                                                     # 120 Hz
    p = plan(FREQS[k:k + 1], max_batch=1)
    try:
        got = p.execute(signals()[:1], out_kind=out)
    finally:
        p.close()
    check(got, of_kind(reference()[:1, k:k + 1], out), TOL * (2 if out == 'power' else 1), f'1 signal, 1 scale {out}')


def test_power_mean_and_itc():
    ref = reference()
    mag = np.abs(ref)
    ref_p = np.mean(mag ** 2, axis=0)
    ref_i = np.abs(np.mean(ref / mag, axis=0))
    good = np.all(mag >= 0.1 * mag.max(axis=-1, keepdims=True), axis=0)
    p = plan(FREQS)
    try:
        pm = p.execute(signals(), out_kind='power_mean')
        itc = p.execute(signals(), out_kind='itc')
    finally:
        p.close()
    check(pm, ref_p, 2e-5, 'power_mean')
    d = np.abs(itc.astype(np.float64) - ref_i)
    dg = d[good].max() if good.any() else 0.0
    print(f'itc: max |d| {d.max():.3e} (1e-3), where every epoch is strong {dg:.3e} (2e-5), {good.mean():.2f} of points')
    assert itc.shape == ref_i.shape and good.any()
    assert dg <= 2e-5 and d.max() <= 1e-3, (dg, d.max())


def test_decimated_call():
    got = nw.Morse(SFREQ, dtype=DTYPE).cwt_batch(signals(), FREQS, decim=4)
    check(got, reference()[..., ::4], TOL, 'decim 4 cwt')
