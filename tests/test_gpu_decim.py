"""GPU tests of time decimation (decim): nw_fused_decim_kernel (nw_decim.hip) through
nw_plan_set_decim, Plan(decim=...) and the decim keyword of the wavelet classes.

A decimated result is the undecimated one [..., ::decim].  The parity cases follow
tests/test_gpu_table_rows.py: complex table rows on hard supports (make_rows), white-noise signals,
the reference oracle.nw_oracle.cwt_from_rows in complex128 sliced [..., ::decim], per signal
max|got - ref| <= 1e-12 (fp64) / 1e-5 (fp32) of max|ref|, doubled for power, and every (signal,
row) reaching 0.25 of its signal's max|ref|, asserted on the reference alone (visible())."""
import ctypes

import numpy as np
import pytest

from epoch_cases import FakeEpochs
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

TOL = {'float64': 1e-12, 'float32': 1e-5}
VISIBLE = 0.25
DTYPES = ['float32', 'float64']
# every supported (n, decim): power-of-two n = 2048 .. 16384, decim >= 2, n / decim >= 1024
PAIRS = [(n, d) for n in (2048, 4096, 8192, 16384) for d in (2, 4, 8, 16) if n // d >= 1024]
KERNEL = 'nw_fused_decim_kernel'
FREQS9 = [1., 7., 40., 120., 250., 330., 420., 470., 499.]   # nine scales: one more than a tile


def noise(S, n, seed, dtype):
    return np.random.default_rng(seed).standard_normal((S, n)).astype(dtype)


def make_rows(supports, length, seed):
    """As tests/test_gpu_table_rows.py: row i complex normal on [0, supports[i]) / sqrt(supports[i])."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((len(supports), length), dtype=np.complex128)
    for i, k in enumerate(supports):
        tab[i, :k] = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.sqrt(k)
    return tab


def reference(x, table, interpolate=False):
    return np.stack([O.cwt_from_rows(xi.astype(np.float64), list(table), interpolate) for xi in x])


def as_kind(c, out):
    return c if out == 'cwt' else np.abs(c) if out == 'abs' else np.abs(c) ** 2


def visible(want):
    top = np.max(np.abs(want), axis=(1, 2))
    worst = np.min(np.max(np.abs(want), axis=2) / top[:, None])
    assert worst >= VISIBLE, f'a row reaches only {worst:.3f} of its signal\'s max|ref|: choose another seed'


def check(got, want, dtype, out, what, factor=1):
    assert got.shape == want.shape, (got.shape, want.shape)
    t = TOL[dtype] * (2 if out == 'power' else 1) * factor
    err = np.max(np.abs(got - want), axis=(1, 2)) / np.max(np.abs(want), axis=(1, 2))
    print(f'{what}: rel err per signal {np.array2string(err, precision=3)} (tol {t:.0e})')
    assert np.all(err <= t), (what, err)


def table_plan(n, dtype, table, max_batch, decim, interpolate=False, **kw):
    F, lf = table.shape
    p = nw.Plan(n, F, dtype, max_batch=max_batch, interpolate=interpolate, decim=decim, **kw)
    p.set_wavelet('table', [], np.arange(1., F + 1), L.nw_grid(1.0, lf, lf), table=table)
    return p


def run_table(n, dtype, table, x, out, max_batch, decim, interpolate=False):
    p = table_plan(n, dtype, table, max_batch, decim, interpolate)
    try:
        got = p.execute(x, out_kind=out)
        st = p.stats()
    finally:
        p.close()
    want_kernel = KERNEL if decim > 1 else 'nw_fused_kernel'
    assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == want_kernel, st
    return got


def fold_supports(n, decim):
    """One fold, exactly one fold's edge, two folds, the last direct fold, the Nyquist bin, the
    mirrored folds and all decim folds."""
    nd = n // decim
    return [nd // 2 + 3, nd, nd + 1, min(n, 2 * nd + 5), n // 2, n // 2 + 1, n - 7, n]


# ------------------------------------------------------------------ 1. parity against the oracle
_parity_ref = {}


def parity_case(n, decim, dtype):
    key = (n, decim, dtype)
    if key not in _parity_ref:
        table = make_rows(fold_supports(n, decim), n, 1100 + n + decim)
        x = noise(11, n, 1200 + n + decim, dtype)          # two signal groups, the second partial
        _parity_ref[key] = (x, table, reference(x, table)[..., ::decim])
    return _parity_ref[key]


@pytest.mark.parametrize('out', ['cwt', 'abs', 'power'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,decim', PAIRS)
def test_decim_parity_every_supported_pair(n, decim, dtype, out):
    assert L.decim_supported(n, L.NW_F32 if dtype == 'float32' else L.NW_F64, decim)
    x, table, ref = parity_case(n, decim, dtype)
    want = as_kind(ref, out)
    assert want.shape == (11, 8, n // decim)
    visible(want)
    got = run_table(n, dtype, table, x, out, max_batch=11, decim=decim)
    check(got, want, dtype, out, f'decim parity n={n} d={decim} {dtype} {out}')


# ------------------------------------------------------------------ 2. analytic rows
@pytest.mark.parametrize('interpolate', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,decim', [(4096, 4), (16384, 16)])
@pytest.mark.parametrize('kind', ['morse', 'morlet'])
def test_decim_analytic_rows(kind, n, decim, dtype, interpolate):
    """Morse (default b, r) and Morlet sigma = 7 at sfreq 1000 against the oracle sliced."""
    x = noise(3, n, 1300 + n, dtype)
    cls = {'morse': nw.Morse, 'morlet': nw.Morlet}[kind]
    w = cls(1000, interpolate=interpolate, dtype=dtype)
    got = w.cwt_batch(x, FREQS9, decim=decim)
    assert [L.KERNEL_NAMES[s['kernel']] for s in w.plan_stats()] == [KERNEL]
    want = np.stack([O.cwt(kind, xi.astype(np.float64), FREQS9, interpolate=interpolate) for xi in x])[..., ::decim]
    check(got, want, dtype, 'cwt', f'{kind} n={n} d={decim} {dtype} interpolate={interpolate}')


# ------------------------------------------------------------------ 3. self-consistency
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,decim', [(2048, 2), (8192, 4), (16384, 2), (16384, 16)])
def test_decim_equals_the_sliced_full_result(n, decim, dtype):
    """The same plan configuration with and without decim, at twice the tolerance (each is within
    one of the reference); power is |cwt|^2 of the decimated cwt."""
    x, table, _ = parity_case(n, decim, dtype)
    full = run_table(n, dtype, table, x, 'cwt', max_batch=11, decim=1)
    dec = run_table(n, dtype, table, x, 'cwt', max_batch=11, decim=decim)
    check(dec, full[..., ::decim], dtype, 'cwt', f'decim vs sliced n={n} d={decim} {dtype}', factor=2)
    pw = run_table(n, dtype, table, x, 'power', max_batch=11, decim=decim)
    c = dec.astype(np.complex128)
    p2 = c.real ** 2 + c.imag ** 2
    # the kernel rounds re^2 + im^2 of the same y twice at most in the compute dtype
    assert np.max(np.abs(pw - p2)) <= 4 * np.finfo(dtype).eps * np.max(p2)


# ------------------------------------------------------------------ 4. chunks
@pytest.mark.parametrize('n,decim,dtype,out', [(4096, 4, 'float32', 'cwt'), (16384, 2, 'float64', 'abs'),
                                               (16384, 8, 'float32', 'power')])
def test_decim_chunks_are_bit_equal(n, decim, dtype, out):
    """S = 11 as chunks of 4, 4, 3 and as one chunk: a row depends on its W row and signal only."""
    x, table, _ = parity_case(n, decim, dtype)
    one = run_table(n, dtype, table, x, out, max_batch=11, decim=decim)
    chunks = run_table(n, dtype, table, x, out, max_batch=4, decim=decim)
    np.testing.assert_array_equal(chunks, one)


# ------------------------------------------------------------------ 5. repeated rows
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind,params,freqs', [('shannon', [], list(range(1, 10))),
                                               ('morse', [17.5, 3.], [5., 5., 9., 5., 9., 9., 5., 40., 40.])])
def test_decim_repeated_rows_match_no_dedup(kind, params, freqs, dtype):
    n, decim, S = 4096, 4, 5
    x = noise(S, n, 1400, dtype)
    g = L.trans_grid(n / 1000., 1000., False)
    res = {}
    for dedup in (True, False):
        p = nw.Plan(n, len(freqs), dtype, max_batch=S, dedup=dedup, decim=decim)
        try:
            p.set_wavelet(kind, params, np.array(freqs, dtype=np.float64), g)
            res[dedup] = [p.execute(x, out_kind=o) for o in ('cwt', 'power')]
            st = p.stats()
        finally:
            p.close()
        assert L.KERNEL_NAMES[st['kernel']] == KERNEL
        assert (st['unique_rows'] < len(freqs)) == dedup, st
    assert res[True][0].shape == (S, len(freqs), n // decim)
    for a, b in zip(res[True], res[False]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 6. epoch reductions
@pytest.mark.parametrize('dtype', DTYPES)
def test_decim_epoch_reductions(dtype):
    """power_mean / itc / power_sum / phase_sum with decim 4 at n = 4096, S = 11 in chunks of 4, 4,
    3, against the reductions of the same plan's materialised decimated cwt (mneutils.py:42-71).
    ITC tolerances of DESIGN.md §2: fp64 1e-10; fp32 2e-5 where every epoch's |cwt| >= 0.1 of its
    row's max, 1e-3 everywhere."""
    n, decim, S = 4096, 4, 11
    f64 = dtype == 'float64'
    x = noise(S, n, 1500, dtype)
    p = nw.Plan(n, len(FREQS9), dtype, max_batch=4, decim=decim)
    try:
        p.set_wavelet('morse', [17.5, 3.], np.array(FREQS9), L.trans_grid(n / 1000., 1000., False))
        res = {}
        for kind in ('power_mean', 'itc', 'power_sum', 'phase_sum', 'cwt'):
            res[kind] = p.execute(x, out_kind=kind)
            assert L.KERNEL_NAMES[p.stats()['kernel']] == KERNEL, kind
    finally:
        p.close()
    pm, itc, ps, ph = res['power_mean'], res['itc'], res['power_sum'], res['phase_sum']
    c = res['cwt'].astype(np.complex128)
    assert c.shape == (S, len(FREQS9), n // decim)
    assert pm.shape == itc.shape == ps.shape == ph.shape == (len(FREQS9), n // decim)
    assert pm.dtype == itc.dtype == np.dtype(dtype) and ps.dtype == np.float64 and ph.dtype == np.complex128
    want_pm = np.mean(np.abs(c) ** 2, axis=0)
    e_pm = np.max(np.abs(pm - want_pm)) / np.max(want_pm)
    mag = np.abs(c)
    d_itc = np.abs(itc.astype(np.float64) - np.abs(np.mean(c / mag, axis=0)))
    good = np.all(mag >= 0.1 * mag.max(axis=-1, keepdims=True), axis=0)
    one = 1e-15 if f64 else 1.2e-7                    # one rounding to the compute dtype
    e_ps = np.max(np.abs(pm - ps / S)) / np.max(np.abs(ps / S))
    e_ph = np.max(np.abs(itc - np.abs(ph) / S))
    print(f'decim reductions {dtype}: power_mean {e_pm:.3e}, itc {d_itc.max():.3e} '
          f'(good {d_itc[good].max() if good.any() else 0.0:.3e}), power_sum/S {e_ps:.3e}, |phase_sum|/S {e_ph:.3e}')
    assert e_pm <= 2 * TOL[dtype]
    if f64:
        assert d_itc.max() <= 1e-10
    else:
        assert good.any() and d_itc[good].max() <= 2e-5 and d_itc.max() <= 1e-3
    assert e_ps <= one and e_ph <= one


# ------------------------------------------------------------------ 7. class API
@pytest.mark.parametrize('dtype', DTYPES)
def test_decim_class_api(dtype):
    n, decim = 4096, 4
    x = noise(3, n, 1600, dtype)
    w = nw.Morse(1000, dtype=dtype)                        # interpolate=False, the class default
    ref = np.stack([O.cwt('morse', xi.astype(np.float64), FREQS9) for xi in x])[..., ::decim]
    for name, fn in (('cwt', w.cwt), ('power', w.power), ('abs', w.abs)):
        got = fn(x[0], FREQS9, decim=decim)
        check(got[None], as_kind(ref[:1], name), dtype, name, f'Morse.{name} decim={decim} {dtype}')
    for out in ('cwt', 'abs', 'power'):
        check(w.cwt_batch(x, FREQS9, out=out, decim=decim), as_kind(ref, out), dtype, out, f'cwt_batch {out} {dtype}')
    assert {L.KERNEL_NAMES[s['kernel']] for s in w.plan_stats()} == {KERNEL}
    full = {o: w.cwt_batch(x, FREQS9, out=o) for o in ('power_mean', 'itc', 'power_sum', 'phase_sum')}
    for o, f in full.items():
        got = w.cwt_batch(x, FREQS9, out=o, decim=decim)
        assert got.shape == (len(FREQS9), n // decim) and got.dtype == f.dtype
        want = f[..., ::decim]
        # twice each contract (both sides are within one of the reference): ITC 1e-10 (fp64) /
        # 1e-3 everywhere (fp32); phase_sum is the sum of 3 such unit phasors;
        # power 2 x 1e-12 / 1e-5 of the maximum
        itc_tol = 2e-10 if dtype == 'float64' else 2e-3
        if o == 'itc':
            assert np.max(np.abs(got - want)) <= itc_tol, o
        elif o == 'phase_sum':
            assert np.max(np.abs(got - want)) <= 3 * itc_tol, o
        else:
            assert np.max(np.abs(got - want)) <= 4 * TOL[dtype] * np.max(np.abs(want)), o


def test_decim_epochs_wavelet():
    """EpochsWavelet.cwt / power / itc with decim against the undecimated calls sliced (twice the
    tolerances: fp64 cwt 1e-12, power 2e-12, ITC 1e-10)."""
    n, decim = 4096, 4
    data = np.random.default_rng(1700).standard_normal((5, 2, n))
    ep = FakeEpochs(data, 1000., ['a', 'b'])
    ew = nw.EpochsWavelet(ep, nw.Morse(1000))
    c, cd = ew.cwt('b', FREQS9), ew.cwt('b', FREQS9, decim=decim)
    assert cd.shape == (5, len(FREQS9), n // decim)
    check(cd, c[..., ::decim], 'float64', 'cwt', 'EpochsWavelet.cwt', factor=2)
    p, pd = ew.power('a', FREQS9), ew.power('a', FREQS9, decim=decim)
    check(pd[None], p[None, :, ::decim], 'float64', 'power', 'EpochsWavelet.power', factor=2)
    i, idec = ew.itc('a', FREQS9), ew.itc('a', FREQS9, decim=decim)
    assert idec.shape == (len(FREQS9), n // decim) and np.max(np.abs(idec - i[:, ::decim])) <= 2e-10
    assert KERNEL in {L.KERNEL_NAMES[s['kernel']] for s in ew.wavelet.plan_stats()}


@pytest.mark.parametrize('n,decim,dtype', [(1201, 5, 'float64'), (32768, 4, 'float32'), (4096, 3, 'float64')])
def test_decim_fallback_lengths(n, decim, dtype):
    """Where nw_decim_supported is false (chirp-z length and a non-divisor, the two-pass form, a
    decim that is no power of two) the full device result is sliced: ceil(n / decim) samples."""
    assert not L.decim_supported(n, L.NW_F32 if dtype == 'float32' else L.NW_F64, decim)
    x = noise(2, n, 1800 + n, dtype)
    freqs = [3., 30., 200.]
    w = nw.Morse(1000, dtype=dtype)
    full = w.cwt_batch(x, freqs)
    got = w.cwt_batch(x, freqs, decim=decim)
    assert got.shape == (2, 3, -(-n // decim)) and got.flags.c_contiguous
    np.testing.assert_array_equal(got, full[..., ::decim])
    np.testing.assert_array_equal(w.power(x[0], freqs, decim=decim), w.power(x[0], freqs)[..., ::decim])
    assert KERNEL not in {L.KERNEL_NAMES[s['kernel']] for s in w.plan_stats()}


def test_decim_fallback_rocfft_engine_and_broadcast_quirk():
    n, decim = 4096, 4
    x = noise(1, n, 1900, 'float64')
    w = nw.Morse(1000, engine='rocfft')
    np.testing.assert_array_equal(w.cwt(x[0], FREQS9, decim=decim), w.cwt(x[0], FREQS9)[..., ::decim])
    assert {s['engine'] for s in w.plan_stats()} == {'rocfft'}
    q = nw.Morse(1000, interpolate=False)
    full = q.power(x[:, :300], range(1, 100))             # the (1, N) form of the README
    got = q.power(x[:, :300], range(1, 100), decim=decim)
    assert got.shape == (99, 75)
    np.testing.assert_array_equal(got, full[..., ::decim])


# ------------------------------------------------------------------ 8. device buffers, plans
def test_decim_device_tensors():
    torch = pytest.importorskip('torch')
    n, decim, S, F = 8192, 4, 5, 8
    x, table, _ = parity_case(n, decim, 'float32')
    x = x[:S]
    p = table_plan(n, 'float32', table, S, decim)
    try:
        assert p.n_out == n // decim
        host = p.execute(x, out_kind='cwt')
        xt = torch.from_numpy(x).cuda()
        ot = torch.empty((S, F, p.n_out), dtype=torch.complex64, device='cuda')
        p.execute(xt, ot, out_kind='cwt')
        p.sync()
        np.testing.assert_array_equal(ot.cpu().numpy(), host)
        pt = torch.empty((F, p.n_out), dtype=torch.float32, device='cuda')
        p.execute(xt, pt, out_kind='power_mean')
        p.sync()
        np.testing.assert_array_equal(pt.cpu().numpy(), p.execute(x, out_kind='power_mean'))
        with pytest.raises(ValueError, match='sizes'):
            p.execute(xt, torch.empty((S, F, n), dtype=torch.complex64, device='cuda'), out_kind='cwt')
        with pytest.raises(ValueError, match='size'):
            p.execute(x, out=np.empty((S, F, n), dtype=np.complex64), out_kind='cwt')
    finally:
        p.close()


def test_decim_multi_plan():
    n, decim, S = 4096, 4, 11
    x, table, _ = parity_case(n, decim, 'float32')
    plans = [table_plan(n, 'float32', table, 8, decim) for _ in range(2)]
    mixed = table_plan(n, 'float32', table, 8, 2)
    try:
        single = plans[0].execute(x, out_kind='power')
        np.testing.assert_array_equal(nw.execute_multi(plans, x, out_kind='power'), single)
        pm = nw.execute_multi(plans, x, out_kind='power_mean')
        assert pm.shape == (8, n // decim)
        want = np.mean(single.astype(np.float64), axis=0)
        assert np.max(np.abs(pm - want)) <= 1.2e-7 * np.max(want)      # one rounding to float32
        with pytest.raises(ValueError, match='decim'):
            nw.execute_multi([plans[0], mixed], x, out_kind='power')
        # ... and by the library itself (check_same_config)
        arr = (ctypes.c_void_p * 2)(plans[0].handle.value, mixed.handle.value)
        out = np.empty((S, 8, n // 2), dtype=np.float32)
        rc = L.lib().nw_execute_multi(arr, 2, x.ctypes.data_as(ctypes.c_void_p), S,
                                      out.ctypes.data_as(ctypes.c_void_p), L.NW_OUT_POWER)
        assert rc == L.NW_E_INVALID and b'decim' in L.lib().nw_last_error()
    finally:
        for p in plans + [mixed]:
            p.close()


def test_decim_ordering_and_unsupported():
    n = 4096
    x, table, _ = parity_case(n, 4, 'float32')
    lib = L.lib()
    p = table_plan(n, 'float32', table, 4, 1)
    try:
        assert lib.nw_plan_set_decim(p.handle, 1) == L.NW_OK                 # a no-op
        assert lib.nw_plan_set_decim(p.handle, 3) == L.NW_E_INVALID          # no power of two
        assert lib.nw_plan_set_decim(p.handle, 8) == L.NW_E_INVALID          # n / decim < 1024
        assert b'decim' in lib.nw_last_error()
        full = p.execute(x[:2], out_kind='cwt')
        assert full.shape == (2, 8, n)
        assert lib.nw_plan_set_decim(p.handle, 2) == L.NW_E_STATE            # after an execute
    finally:
        p.close()
    with pytest.raises(ValueError):
        nw.Plan(n, 8, 'float32', decim=3)
    with pytest.raises(ValueError):
        nw.Plan(1000, 8, 'float32', decim=2)
    with pytest.raises(ValueError):
        nw.Plan(32768, 8, 'float32', decim=2)
    with pytest.raises(ValueError, match='rocFFT'):
        nw.Plan(n, 8, 'float32', engine='rocfft', decim=2)
