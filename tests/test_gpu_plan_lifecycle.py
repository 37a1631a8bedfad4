"""A plan that has been used gives what a fresh plan gives.

The drop-in classes keep one plan per (n, F, dtype, ...) and re-arm it with nw_plan_set_wavelet
whenever the cache changes (WaveletBase._plan), and one plan serves every output kind and batch
size.  nw_plan_set_wavelet has to drop everything the previous wavelet left behind (the W table
and its supports, the two-pass supports, the chirp-z M classes, the repeated-row and overflow
views, the table and its row lengths, the form a tentative chirp-z length settled on), and
every execute has to start from clean accumulators.

The principle tested: after any history a plan gives BIT FOR BIT what a fresh plan gives for the
same wavelet, input and output kind (assert_array_equal on equal NaN masks and finite values:
the kernels are deterministic, tests/test_gpu_timing_paths.py), and its cwt meets the parity
contract against oracle.nw_oracle per signal: max|got - ref| <= 1e-12 (fp64) / 1e-5 (fp32) of
max|ref| (tests/test_gpu_parity.py), 2e-5 for fp32 on the chirp-z form (tests/test_gpu_chirp.py)."""
import numpy as np
import pytest

from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

SFREQ = 1000.
F = 6
# (id, n, dtype, engine): the forms a plan can take
FORMS = [('one-pass-pair', 2048, 'float32', None), ('one-pass-e32', 8192, 'float64', None),
         ('two-pass', 1 << 15, 'float32', None), ('two-pass', 1 << 15, 'float64', None),
         ('chirp', 1201, 'float32', None), ('chirp', 1201, 'float64', None),
         ('rocfft', 2048, 'float32', 'rocfft')]
ONE_DTYPE = [FORMS[0], FORMS[1], FORMS[2], FORMS[5], FORMS[6]]
ENGINE_OF = {'one-pass-pair': 'fused', 'one-pass-e32': 'fused', 'two-pass': 'fused', 'chirp': 'fused',
             'rocfft': 'rocfft'}
EXTRA_KINDS = ['power', 'abs', 'power_mean', 'itc', 'power_sum', 'phase_sum']


def form_id(c):
    return f'{c[0]}-{c[1]}-{c[2]}'


def signals(S, n, seed, dtype):
    """An offset, one slow and one fast sinusoid and white noise: every wavelet below, from
    Shannon's <= 1 Hz rows to Morse at 450 Hz, sees signal."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SFREQ
    lo, hi = rng.uniform(1, 6, (S, 1)), rng.uniform(60, 450, (S, 1))
    ph = rng.uniform(0, 2 * np.pi, (2, S, 1))
    x = (0.5 + np.sin(2 * np.pi * lo * t + ph[0]) + np.sin(2 * np.pi * hi * t + ph[1])
         + 0.3 * rng.standard_normal((S, n)))
    return x.astype(dtype)


def same_bits(a, b, what):
    """Equal NaN masks and equal values elsewhere."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb, err_msg=f'{what}: NaN masks differ')
    np.testing.assert_array_equal(a[~na], b[~nb], err_msg=what)


def contract(got, ref, dtype, form, what):
    t = 1e-12 if dtype == 'float64' else (2e-5 if form == 'chirp' else 1e-5)
    err = np.max(np.abs(got - ref), axis=(1, 2)) / np.max(np.abs(ref), axis=(1, 2))
    print(f'{what}: rel err per signal {np.array2string(err, precision=3)} (tol {t:.0e})')
    assert np.all(err <= t), (what, err)


# ------------------------------------------------------------------ the wavelets of a sequence
def user_table(n, seed, equal_rows=False):
    rng = np.random.default_rng(seed)
    row_len = [n] * F if equal_rows else [n, n - 1, n - 8, n // 2, 100, n - 3]
    tab = np.zeros((F, n), dtype=np.complex128)
    for i, m in enumerate(row_len):
        tab[i, :m] = (rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(m)
    if equal_rows:
        tab[:] = tab[0]
    return tab, row_len


def wavelet_steps(n):
    """(name, set_wavelet arguments, expected unique_rows, oracle(x) -> (F, n))."""
    grid = L.trans_grid(n / SFREQ, SFREQ, False)
    short = L.trans_grid(n / 2000., SFREQ, False)
    nu_short = O.trans_grid(SFREQ, n / 2000., False)
    assert short.len_full == len(nu_short) < n
    narrow, wide = np.arange(1., 7.), np.linspace(60., 450., F)
    f_morlet = np.array([2., 9., 40., 90., 200., 350.])
    f_rep = np.array([5., 5., 5., 80., 80., 80.])
    f_short = np.array([3., 10., 30., 80., 150., 300.])
    f_hat = np.arange(1., 100., 7.)[:F]
    tab_g, len_g = user_table(n, 11)
    tab_i, len_i = user_table(n, 12, equal_rows=True)
    tgrid = L.nw_grid(1.0, n, n)

    def morse(freqs):
        return lambda x: O.cwt('morse', x, freqs)

    def table(tab, row_len):
        return lambda x: O.cwt_from_rows(x, [tab[i, :m] for i, m in enumerate(row_len)], False)

    a = ('a: morse narrow', dict(kind='morse', params=[17.5, 3.], freqs=narrow, grid=grid), F, morse(narrow))
    return [
        a,
        ('b: morse wide', dict(kind='morse', params=[17.5, 3.], freqs=wide, grid=grid), F, morse(wide)),
        ('c: morlet', dict(kind='morlet', params=[7., 0.], freqs=f_morlet, grid=grid), F,
         lambda x: O.cwt('morlet', x, f_morlet, sigma=7., gabor=False)),
        ('d: shannon', dict(kind='shannon', params=[], freqs=narrow, grid=grid), 1,
         lambda x: O.cwt('shannon', x, narrow)),
        ('e: morse repeated', dict(kind='morse', params=[17.5, 3.], freqs=f_rep, grid=grid), 2, morse(f_rep)),
        ('f: morse short grid', dict(kind='morse', params=[17.5, 3.], freqs=f_short, grid=short), F,
         lambda x: O.cwt_from_rows(x, [O.morse_spectrum(nu_short, f) for f in f_short], False)),
        ('g: user table ragged',
         dict(kind='table', params=[], freqs=narrow, grid=tgrid, table=tab_g, row_len=len_g), F,
         table(tab_g, len_g)),
        ('h: mexican hat',
         dict(kind='mexican_hat', params=[7., SFREQ, 1.], freqs=f_hat, grid=L.nw_grid(1.0, 0, 0)), F,
         lambda x: O.cwt('mexican_hat', x, f_hat)),
        ('i: user table equal rows',
         dict(kind='table', params=[], freqs=narrow, grid=tgrid, table=tab_i, row_len=len_i), 1,
         table(tab_i, len_i)),
        a,
    ]


# ------------------------------------------------------------------ 1. wavelet replacement
@pytest.mark.parametrize('form,n,dtype,engine', FORMS, ids=[form_id(c) for c in FORMS])
def test_replace_wavelet_on_a_live_plan(form, n, dtype, engine):
    """Ten wavelets in a row on one plan (narrow and wide supports, every kind, repeated rows,
    a shorter cache grid, user and device-built tables), S = 3 in chunks of 2 + 1: after each
    set_wavelet the cwt and one more output kind (rotating through all six) equal a fresh
    plan's bit for bit, the stats agree, and the cwt meets the oracle's contract."""
    S = 3
    x = signals(S, n, 40 + n, dtype)
    x64 = x.astype(np.float64)
    live = nw.Plan(n, F, dtype, max_batch=2, engine=engine)
    try:
        for i, (name, args, uniq, oracle) in enumerate(wavelet_steps(n)):
            extra = EXTRA_KINDS[i % len(EXTRA_KINDS)]
            what = f'{form} n={n} {dtype} step {name}'
            fresh = nw.Plan(n, F, dtype, max_batch=2, engine=engine)
            try:
                res = []
                for p in (live, fresh):
                    p.set_wavelet(**args)
                    res.append((p.execute(x, out_kind='cwt'), p.execute(x, out_kind=extra), p.stats()))
            finally:
                fresh.close()
            (lc, le, ls), (fc, fe, fs) = res
            same_bits(lc, fc, f'{what}: cwt')
            same_bits(le, fe, f'{what}: {extra}')
            assert ls['unique_rows'] == fs['unique_rows'] == uniq, (what, ls['unique_rows'], fs['unique_rows'])
            assert ls['engine'] == fs['engine'] == ENGINE_OF[form], (what, ls['engine'], fs['engine'])
            contract(lc, np.stack([oracle(xi) for xi in x64]), dtype, form, what)
    finally:
        live.close()


# ------------------------------------------------------------------ 2. a tentative chirp-z length
def chirp_synth(S, n, seed):
    """synth of tests/test_gpu_chirp.py plus an offset and a 0.5 Hz component (Shannon's rows
    pass <= 1 Hz only)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SFREQ
    fc = rng.uniform(1, 100, (S, 1))
    ph = rng.uniform(0, 2 * np.pi, (S, 1))
    return (0.5 + np.sin(2 * np.pi * 0.5 * t) + np.sin(2 * np.pi * fc * t + ph)
            + 0.1 * rng.standard_normal((S, n))).astype(np.float32)


def chirp_within(got, ref, dtype, out):
    """within of tests/test_gpu_chirp.py."""
    t = (1e-12 if dtype == 'float64' else 2e-5) * (2 if out == 'power' else 1)
    floor = 1e-30 if dtype == 'float32' else 0.0
    return np.max(np.abs(got - ref), initial=0.0) <= t * np.max(np.abs(ref), initial=0.0) + floor


@pytest.mark.parametrize('dtype,n', [('float32', 10001), ('float64', 5001)])
def test_tentative_length_rearms_on_the_same_plan(dtype, n):
    """2n - 1 beyond the largest on-chip transform (test_chirp_tentative_lengths), every step on
    ONE plan: narrow rows (chirp-z) -> no row fits (rocFFT) -> narrow again (chirp-z again) ->
    hybrid -> no row fits -> Shannon."""
    S = 2
    x = chirp_synth(S, n, 55).astype(dtype)
    x64 = x.astype(np.float64)
    g = L.trans_grid(n / SFREQ, SFREQ, False)
    narrow, allwide, hybrid = np.array([2., 5., 11.]), np.array([300., 350., 400.]), np.array([2., 5., 400.])
    steps = [('narrow', 'morse', narrow, 'fused'), ('all wide', 'morse', allwide, 'rocfft'),
             ('narrow again', 'morse', narrow, 'fused'), ('hybrid', 'morse', hybrid, 'fused'),
             ('all wide again', 'morse', allwide, 'rocfft'), ('shannon', 'shannon', narrow, 'fused')]
    live = nw.Plan(n, 3, dtype, max_batch=2)
    try:
        for name, kind, freqs, engine in steps:
            params = [17.5, 3.] if kind == 'morse' else []
            ref = np.stack([O.cwt(kind, xi, freqs) for xi in x64])
            fresh = nw.Plan(n, 3, dtype, max_batch=2)
            try:
                for p in (live, fresh):
                    p.set_wavelet(kind, params, freqs, g)
                for out in ('power', 'cwt'):
                    a, b = live.execute(x, out_kind=out), fresh.execute(x, out_kind=out)
                    assert live.stats()['engine'] == fresh.stats()['engine'] == engine, (name, out)
                    same_bits(a, b, f'n={n} {dtype} {name}: {out}')
                    want = ref if out == 'cwt' else np.abs(ref) ** 2
                    err = np.max(np.abs(a - want)) / np.max(np.abs(want))
                    assert chirp_within(a, want, dtype, out), (name, out, err)
                assert live.stats()['unique_rows'] == fresh.stats()['unique_rows']
            finally:
                fresh.close()
    finally:
        live.close()


# ------------------------------------------------------------------ 3. execute history
CALLS = [('cwt', 5), ('power_mean', 5), ('power_mean', 5), ('abs', 1), ('itc', 9), ('power', 8), ('phase_sum', 3),
         ('power_mean', 0), ('power_sum', 9), ('cwt', 2)]
DEVICE_CALLS = (0, 4, 8)      # repeated with device tensors on the live plan


def device_execute(torch, plan, x, kind, like):
    xt = torch.from_numpy(x).cuda()
    ot = torch.empty(like.shape, dtype=getattr(torch, str(like.dtype)), device='cuda')
    plan.execute(xt, ot, out_kind=kind)
    plan.sync()
    return ot.cpu().numpy()


@pytest.mark.parametrize('form,n,dtype,engine', ONE_DTYPE, ids=[form_id(c) for c in ONE_DTYPE])
def test_execute_history_does_not_matter(form, n, dtype, engine):
    """Output kinds, batch sizes (whole chunks, ragged ones, none) and reductions in sequence on
    one plan: each result equals bit for bit that of a fresh plan making only that call; the
    repeated power_mean equals the first (the accumulators start from zero); device-tensor
    executes in between equal the host ones."""
    try:
        import torch
    except ImportError:
        torch = None
    x = signals(9, n, 70 + n, dtype)
    freqs = np.arange(1., 7.)
    g = L.trans_grid(n / SFREQ, SFREQ, False)

    def plan():
        p = nw.Plan(n, F, dtype, max_batch=4, engine=engine)
        p.set_wavelet('morse', [17.5, 3.], freqs, g)
        return p

    live = plan()
    try:
        results = []
        for i, (kind, S) in enumerate(CALLS):
            what = f'{form} n={n} {dtype} call {i + 1} ({kind}, {S})'
            got = live.execute(x[:S], out_kind=kind)
            fresh = plan()
            try:
                want = fresh.execute(x[:S], out_kind=kind)
            finally:
                fresh.close()
            same_bits(got, want, what)
            if S == 0:
                assert np.all(np.isnan(got)), what
            else:
                assert np.all(np.isfinite(got)) and np.any(got != 0), what
            if torch is not None and i in DEVICE_CALLS:
                same_bits(device_execute(torch, live, x[:S], kind, got), got, f'{what}: device tensors')
            results.append(got)
        same_bits(results[2], results[1], f'{form} n={n} {dtype}: the repeated power_mean')
    finally:
        live.close()


# ------------------------------------------------------------------ 4. the class path
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('cls,kind', [(nw.Morse, 'morse'), (nw.MexicanHat, 'mexican_hat')])
def test_class_reuses_its_plan_for_new_freqs(cls, kind, dtype):
    """w.cwt(x, other_freqs, reuse=False) re-arms the object's one cached plan (MexicanHat: the
    device-built table is rebuilt, its row lengths change with the freqs): each result equals a
    new object's first call bit for bit and meets the oracle's contract."""
    n = 4096
    x = signals(1, n, 90, dtype)[0]
    x64 = x.astype(np.float64)
    f1, f2, f3 = [1., 2., 3., 4., 5., 6.], [60., 138., 216., 294., 372., 450.], [2., 5., 11., 80., 200., 400.]
    w = cls(SFREQ, dtype=dtype)
    calls = [('cwt', f1, f1), ('cwt', f2, f2), ('power', f3, f3), ('cwt', None, f3)]
    for i, (op, arg, freqs) in enumerate(calls):
        what = f'{kind} {dtype} call {i + 1} ({op})'
        got = getattr(w, op)(x, arg, reuse=False) if arg is not None else getattr(w, op)(x, None)
        assert len(w._plans) == 1, what
        new = getattr(cls(SFREQ, dtype=dtype), op)(x, freqs)
        same_bits(got, new, what)
        ref = O.cwt(kind, x64, freqs)
        t = (1e-12 if dtype == 'float64' else 1e-5) * (2 if op == 'power' else 1)
        want = ref if op == 'cwt' else np.abs(ref) ** 2
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f'{what}: rel err {err:.3e} (tol {t:.0e})')
        assert err <= t, (what, err)
