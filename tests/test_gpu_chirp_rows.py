"""GPU parity of the chirp-z kernel (nw_chirp.hip) per row, at every transform size M, elements per
thread E, pass-0 variant NZ and kind of W row, and at the corners of chirp_class (nw_shape.h).
tests/test_gpu_chirp.py covers the lengths and the plan logic with narrowband signals under one
maximum over all rows; here the signals are white noise, every row is checked against a maximum it
reaches, and which (M, E, NZ) each row takes is predicted with tests/chirp_variants.py (pinned to
the header by tests/test_host_asan.py) and asserted, with the number of kernel launches.

Reference: oracle.nw_oracle.cwt_from_rows in complex128 on the rows the plan holds (|.| and |.|^2
taken from it; the epoch sums formed from it in fp64 in signal order).  Bound, per signal: the
contract of tests/test_gpu_chirp.py, max|got - ref| <= 1e-12 (fp64) / 2e-5 (fp32) of max|ref| over
the checked rows, doubled for |.|^2; every checked (signal, row) reaches 0.25 of that maximum,
asserted on the reference alone (visible()).  Rows that cannot (a one-bin row, the smooth rows of
part d) are held to their own maximum.  Every execute asserts the fused engine, nw_chirp_kernel,
no rocFFT multiply unless a row is off chip on purpose, and launches_fused growing by (distinct
predicted M) x (chunks).

  a. complex table rows at n = M / 2 + 1, where every K <= M / 2 is in class M: K = 1, TT, TT + 1,
     2 TT, 2 TT + 1, 4 TT, 4 TT + 1 (TT = M / E: each NZ of {1, 2, 4, E / 2} at both ends of its
     bucket) and M / 2 (2K == M and n + K - 1 == M at once), K = n (class 2M; through rocFFT at
     the largest M, where the length is tentative) and an all-zero row (exact zeros);
  b. the tight wrap at n = M / 2 + 200, where one aliased lag is >= 1e-3 of the row's maximum
     (tests/test_chirp_cpu.py): K = M - n + 1, the last in class M, and K + 1, as table rows of one
     plan and as Shannon rows;
  c. real rows (REALW kernels) with a hard edge: Shannon plans on a grid of spacing
     1 / (K - 0.5), whose row is 1 on [0, K), one plan per K of (a) (the plan API takes such a grid);
  d. Morse (17.5, 3) and Morlet (7, 0) at n = 1201, 1000, 3000, 4097 with rows in every class the
     length reaches, plain and interpolated, each row against its own maximum;
  e. power_sum and phase_sum at n = M / 2 - 1 (not tentative, every K >= 3 in class M) in chunks of
     11 and of 4, 4, 3: bit-identical, reduce_path as chirp_variants.psum_ok says.

Measured under (d): no row over the contract bound (test_smooth_rows_in_several_classes)."""
import numpy as np
import pytest

import chirp_variants as V
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

TOL = {'float64': 1e-12, 'float32': 2e-5}
VISIBLE = 0.25
OUTS = ['cwt', 'abs', 'power']
SIZES = [('float32', m) for m in V.CLASSES] + [('float64', m) for m in V.CLASSES[:4]]


def as_kind(c, out):
    return c if out == 'cwt' else np.abs(c) if out == 'abs' else np.abs(c) ** 2


def reference(x, rows):
    """(S, F, n) complex128 of the rows (F, n) as the plan holds them."""
    return np.stack([O.cwt_from_rows(xi.astype(np.float64), list(rows), False) for xi in x])


def visible(want, rows):
    """The 0.25 condition on the reference: each of ``rows`` reaches VISIBLE of its signal's max
    over ``rows``."""
    per_row = np.max(np.abs(want[:, rows]), axis=2)
    worst = np.min(per_row / np.max(per_row, axis=1, keepdims=True))
    assert worst >= VISIBLE, f'a row reaches only {worst:.3f} of its signal\'s max|ref|: choose another seed'


def check(got, want, dtype, out, what, rows):
    """Per signal, over ``rows``: max|got - want| <= tol x max|want|."""
    assert got.shape == want.shape, (got.shape, want.shape)
    t = TOL[dtype] * (2 if out == 'power' else 1)
    g, w = got[:, rows], want[:, rows]
    err = np.max(np.abs(g - w), axis=(1, 2)) / np.max(np.abs(w), axis=(1, 2))
    print(f'{what}: rel err per signal {np.array2string(err, precision=3)} (tol {t:.0e})')
    assert np.all(err <= t), (what, err)


def predict(n, supports, dtype, out):
    """[(M, NZ)] of rows of the given supports for the kernel that writes ``out``; (-1, 0): off chip."""
    res = []
    for k in supports:
        m = V.chirp_class(n, k, dtype)
        res.append((m, V.pass0_nz(k, m, V.chirp_e(m, dtype, out))) if m > 0 else (-1, 0))
    return res


def execute(p, x, out, classes, chunks, off_chip=False):
    """One execute with the assertions every run makes: ``classes`` are the predicted transform
    sizes of the rows on chip."""
    before = p.stats()
    got = p.execute(x, out_kind=out)
    st = p.stats()
    assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'nw_chirp_kernel', st
    grown = st['launches_fused'] - before['launches_fused']
    assert grown == len(set(classes)) * chunks, (grown, sorted(set(classes)), chunks)
    mult = st['launches_multiply'] - before['launches_multiply']
    assert (mult > 0) if off_chip else (mult == 0), (mult, off_chip)
    return got, st


def table_plan(n, dtype, table, max_batch):
    p = nw.Plan(n, len(table), dtype, max_batch=max_batch)
    p.set_wavelet('table', [], np.arange(1., len(table) + 1), L.nw_grid(1.0, n, n), table=table)
    return p


def shannon_plan(n, dtype, k, max_batch):
    """F = 1 (no repeated-row view): the row is 1 on [0, k)."""
    p = nw.Plan(n, 1, dtype, max_batch=max_batch)
    p.set_wavelet('shannon', [], np.array([1.0]), L.nw_grid(V.shannon_delta(k), n, n))
    return p


def corner_supports(m, dtype, out):
    """The K of part (a): both ends of every pass-0 bucket of the kernel that writes ``out``."""
    tt = m // V.chirp_e(m, dtype, out)
    return [1, tt, tt + 1, 2 * tt, 2 * tt + 1, 4 * tt, 4 * tt + 1, m // 2]


# ------------------------------------------------------------------ a. complex rows
_table_ref = {}


def table_case(n, dtype, supports, seed):
    key = (n, dtype, tuple(supports))
    if key not in _table_ref:
        table = V.hard_rows(supports, n, seed)
        x = V.noise(3, n, seed + 1, dtype)
        _table_ref[key] = (x, table, reference(x, table))
    return _table_ref[key]


@pytest.mark.parametrize('out', OUTS)
@pytest.mark.parametrize('dtype,m', SIZES)
def test_table_rows_every_class_and_variant(dtype, m, out):
    """F = 10 at n = M / 2 + 1, S = 3 in one chunk.  Rows 0-7: the corners, all in class M, variants
    {1, 2, 4, E / 2}; row 8: K = n, class 2M, or off chip through rocFFT at the largest M; row 9:
    all zero (class M, NZ = 1), exact zeros."""
    n = m // 2 + 1
    top = m == V.chirp_mmax(dtype)
    e = V.chirp_e(m, dtype, out)
    supports = corner_supports(m, dtype, out) + [n, 0]
    x, table, ref = table_case(n, dtype, supports, 100 + m)
    assert [V.table_support(r) for r in table] == supports
    pred = predict(n, supports, dtype, out)
    assert [c for c, _ in pred] == [m] * 8 + [-1 if top else 2 * m, m], pred
    assert [v for _, v in pred[:8]] == [1, 1, 2, 2, 4, 4, e // 2, e // 2], pred
    assert {v for _, v in pred[:8]} == {1, 2, 4, e // 2} and pred[9] == (m, 1)
    assert n + supports[7] - 1 == m and 2 * supports[7] == m
    want = as_kind(ref, out)
    full = np.arange(1, 9)
    visible(want, full)
    assert np.all(want[:, 9] == 0) and np.all(np.max(np.abs(want[:, 0]), axis=-1) > 0)
    p = table_plan(n, dtype, table, 3)
    try:
        got, _ = execute(p, x, out, [c for c, _ in pred if c > 0], 1, off_chip=top)
    finally:
        p.close()
    check(got, want, dtype, out, f'corners M={m} {dtype} {out}', full)
    check(got, want, dtype, out, f'one-bin row M={m} {dtype} {out}', slice(0, 1))
    assert np.all(got[:, 9] == 0), 'the all-zero row must give exact zeros'


# ------------------------------------------------------------------ b. the tight wrap
_shannon_ref = {}


def shannon_case(n, dtype, k, seed):
    key = (n, dtype, k)
    if key not in _shannon_ref:
        row = V.shannon_row(V.shannon_delta(k), n)
        assert V.table_support(row) == k == V.shannon_support(V.shannon_delta(k), n) and np.all(row[:k] == 1)
        x = V.noise(3, n, seed, dtype)
        _shannon_ref[key] = (x, reference(x, row[None].astype(np.complex128)))
    return _shannon_ref[key]


@pytest.mark.parametrize('out', OUTS)
@pytest.mark.parametrize('dtype,m', SIZES)
def test_tight_wrap_where_one_bin_shows(dtype, m, out):
    """n = M / 2 + 200: K = M - n + 1 runs at M with no lag to spare, K + 1 at 2M -- or, at the
    largest M, off chip: the table plan then runs that row through rocFFT, and the Shannon plan,
    whose only row it is, runs on the rocFFT engine.  All against the same reference."""
    n, kb = V.wrap_case(m)
    top = m == V.chirp_mmax(dtype)
    supports = [kb, kb + 1]
    pred = predict(n, supports, dtype, out)
    assert [c for c, _ in pred] == [m, -1 if top else 2 * m] and n + kb - 1 == m
    x, table, ref = table_case(n, dtype, supports, 300 + m)
    want = as_kind(ref, out)
    visible(want, np.arange(2))
    p = table_plan(n, dtype, table, 3)
    try:
        got, _ = execute(p, x, out, [c for c, _ in pred if c > 0], 1, off_chip=top)
    finally:
        p.close()
    check(got, want, dtype, out, f'wrap table M={m} {dtype} {out}', np.arange(2))
    for k, (c, _) in zip(supports, pred):
        xs, sref = shannon_case(n, dtype, k, 400 + m)
        swant = as_kind(sref, out)
        p = shannon_plan(n, dtype, k, 3)
        try:
            if c > 0:
                got, _ = execute(p, xs, out, [c], 1)
            else:
                got = p.execute(xs, out_kind=out)
                assert p.stats()['engine'] == 'rocfft'
        finally:
            p.close()
        check(got, swant, dtype, out, f'wrap shannon K={k} M={m} {dtype} {out}', np.arange(1))


# ------------------------------------------------------------------ c. real rows with a hard edge
@pytest.mark.parametrize('out', OUTS)
@pytest.mark.parametrize('dtype,m', SIZES)
def test_real_rows_every_variant(dtype, m, out):
    """The REALW kernels at n = M / 2 + 1: one Shannon plan (F = 1) per K of part (a), its row 1 on
    [0, K); together the plans take every variant of {1, 2, 4, E / 2} in class M."""
    n = m // 2 + 1
    e = V.chirp_e(m, dtype, out)
    supports = corner_supports(m, dtype, out)
    pred = predict(n, supports, dtype, out)
    assert pred == [(m, v) for v in (1, 1, 2, 2, 4, 4, e // 2, e // 2)], pred
    for k in supports:
        x, ref = shannon_case(n, dtype, k, 500 + m)
        p = shannon_plan(n, dtype, k, 3)
        try:
            got, _ = execute(p, x, out, [m], 1)
        finally:
            p.close()
        check(got, as_kind(ref, out), dtype, out, f'shannon K={k} M={m} {dtype} {out}', np.arange(1))


# ------------------------------------------------------------------ d. smooth rows
CANDIDATES = [2, 3, 4, 6, 8, 10, 12, 15, 20, 25, 30, 40, 50, 60, 70, 80, 90, 100, 120, 150, 180, 200, 220, 250, 300,
              350, 400, 450, 500, 600, 2000]
KIND_KW = {'morse': {}, 'morlet': {'sigma': 7., 'gabor': False}}
KIND_PARAMS = {'morse': (17.5, 3.), 'morlet': (7., 0.)}


def analytic_rows(kind, n, freqs, interpolate):
    """(F, n) float64: the oracle's rows of the analytic kind at sfreq = 1000, padded to n."""
    rows = O.fft_wavelets(kind, list(freqs), 1000., n / 1000., interpolate, **KIND_KW[kind])
    return np.array([O.pad_to(r, n) for r in rows])


def soft_support(row, n, dtype):
    """(K_lo, K_hi, hard) of an analytic row: K of the oracle row rounded to the dtype (with and
    without the 1 / n the table folds in); in fp32 also with values below 2^-126 flushed, as the
    kernels' exponentials do.  hard: the last bin is O(1) of the row's maximum (a full row, or the
    interpolate cut), so K is certain."""
    ks = [V.table_support(row.astype(dtype)), V.table_support((row / n).astype(dtype))]
    if dtype == 'float32':
        ks.append(V.table_support(np.where(np.abs(row) < 2.0 ** -126, 0.0, row)))
    k = ks[0]
    hard = k > 0 and abs(row[k - 1]) >= 1e-3 * np.max(np.abs(row))
    return min(ks), max(ks), hard


def certain(n, row, dtype, outs):
    """The (M, NZ per out) of an analytic row if its predicted support sits at least 10 % of the
    pass-0 bucket M / E away from every class and variant boundary, for every kernel of ``outs``;
    else None."""
    lo, hi, hard = soft_support(row, n, dtype)
    res = []
    for out in outs:
        m = V.chirp_class(n, lo, dtype)
        e = V.chirp_e(m, dtype, out) if m > 0 else 0
        if e == 0:
            return None
        margin = 0 if hard else m // e // 10 + 1
        seen = {predict(n, [k], dtype, out)[0] for k in (max(lo - margin, 0), lo, hi, min(hi + margin, n))}
        if len(seen) != 1:
            return None
        res.append(seen.pop())
    assert len({c for c, _ in res}) == 1
    return res[0][0], tuple(v for _, v in res)


def choose_freqs(kind, n, dtype, outs, want_classes=None, limit=10):
    """Up to two candidates per (M, NZ) bucket, ascending, at most ``limit``: decided on the
    reference rows alone."""
    rows = analytic_rows(kind, n, CANDIDATES, False)
    buckets = {}
    for f, row in zip(CANDIDATES, rows):
        c = certain(n, row, dtype, outs)
        if c is not None and (want_classes is None or c[0] in want_classes) and len(buckets.setdefault(c, [])) < 2:
            buckets[c].append(f)
    picked = sorted((f, c) for c, fs in buckets.items() for f in fs)
    while len(picked) > limit:                       # thin the fullest bucket
        counts = {}
        for _, c in picked:
            counts[c] = counts.get(c, 0) + 1
        worst = max(counts, key=lambda c: (counts[c], c))
        picked.remove(next(fc for fc in picked if fc[1] == worst))
    return [float(f) for f, _ in picked], [c for _, c in picked]


def reachable_classes(n, dtype):
    return {V.chirp_class(n, k, dtype) for k in range(1, n + 1)} - {-1}


def row_errors(got, want):
    """(S, F): each row's max|got - want| over its own max|want|."""
    return np.max(np.abs(got - want), axis=2) / np.max(np.abs(want), axis=2)


SMOOTH = [(1201, 'float32'), (1201, 'float64'), (1000, 'float32'), (1000, 'float64'), (3000, 'float32'),
          (3000, 'float64'), (4097, 'float32')]


@pytest.mark.parametrize('kind', ['morse', 'morlet'])
@pytest.mark.parametrize('n,dtype', SMOOTH)
def test_smooth_rows_in_several_classes(n, dtype, kind):
    """8-10 frequencies whose rows together take every class the length reaches, each predicted
    support clear of the class and variant boundaries (certain()); S = 3; cwt, abs and power, and
    once more with interpolate.  Each (signal, row) is held to its own maximum at the contract
    bound, or -- printed when it applies -- to twice the error of the rocFFT engine (independent
    code, same dtype, same inputs) against the same reference where that is larger.  Measured on
    an MI355X: the allowance never applied; the worst row is at 4.1e-6 (fp32) and 8.0e-15 (fp64) of
    its maximum."""
    freqs, pred = choose_freqs(kind, n, dtype, OUTS)
    assert 8 <= len(freqs) <= 10, (freqs, pred)
    assert {c for c, _ in pred} == reachable_classes(n, dtype), (pred, reachable_classes(n, dtype))
    x = V.noise(3, n, 700 + n, dtype)
    for interp in (False, True):
        rows = analytic_rows(kind, n, freqs, interp)
        if interp:
            cs = [certain(n, r, dtype, OUTS) for r in rows]
            keep = [i for i, c in enumerate(cs) if c is not None]
            assert len(keep) >= 6, cs
            classes = [cs[i][0] for i in keep]
        else:
            keep, classes = list(range(len(freqs))), [c for c, _ in pred]
        fk = np.array([freqs[i] for i in keep])
        ref = np.stack([O.cwt_from_rows(xi.astype(np.float64), list(rows[keep]), interp) for xi in x])
        g = L.trans_grid(n / 1000., 1000., interp)
        p = nw.Plan(n, len(fk), dtype, max_batch=3, interpolate=interp)
        q = nw.Plan(n, len(fk), dtype, max_batch=3, interpolate=interp, engine='rocfft')
        try:
            p.set_wavelet(kind, list(KIND_PARAMS[kind]), fk, g)
            q.set_wavelet(kind, list(KIND_PARAMS[kind]), fk, g)
            for out in OUTS:
                want = as_kind(ref, out)
                got, _ = execute(p, x, out, classes, 1)
                other = q.execute(x, out_kind=out)
                assert q.stats()['engine'] == 'rocfft'
                t = TOL[dtype] * (2 if out == 'power' else 1)
                err, base = row_errors(got, want), row_errors(other, want)
                allowed = np.maximum(t, 2 * base)
                print(f'smooth {kind} n={n} {dtype} interp={interp} {out}: worst row err {err.max():.3e} '
                      f'(contract {t:.0e}; rocFFT engine {base.max():.3e}; rows over the contract: '
                      f'{int(np.sum(err > t))})')
                assert np.all(err <= allowed), (out, interp, err.max(), base.max())
        finally:
            p.close()
            q.close()


# ------------------------------------------------------------------ e. epoch sums
def sums_of(ref):
    """power_sum (F, n) and phase_sum (F, n) complex of the reference, added in signal order."""
    ps = np.zeros(ref.shape[1:])
    ph = np.zeros(ref.shape[1:], dtype=np.complex128)
    for y in ref:
        ps += np.abs(y) ** 2
        ph += y / np.abs(y)
    return ps, ph


def check_sums(res, ref, dtype, what):
    S = ref.shape[0]
    ps, ph = sums_of(ref)
    t = 2 * TOL[dtype]
    e_ps = np.max(np.abs(res['power_sum'] - ps), axis=1) / np.max(np.abs(ps), axis=1)
    d = np.abs(res['phase_sum'] - ph)
    mag = np.abs(ref)
    good = np.all(mag >= 0.1 * mag.max(axis=-1, keepdims=True), axis=0)
    assert good.mean() >= 0.2, good.mean()
    print(f'{what}: power_sum rel err per row {e_ps.max():.3e} (tol {t:.0e}), phase_sum abs err {d.max():.3e} '
          f'(good points {d[good].max():.3e}, {good.mean():.0%} of them)')
    assert np.all(e_ps <= t), e_ps
    if dtype == 'float64':
        assert d.max() <= 1e-10 * S, d.max()
    else:
        assert d[good].max() <= 2e-5 * S and d.max() <= 1e-3 * S, (d[good].max(), d.max())


def run_sums(make, x, dtype, m, classes):
    """power_sum and phase_sum of a plan at max_batch 11 (one chunk, blocks of 8 + 3) and 4 (chunks
    4, 4, 3): reduce_path as psum_ok says, the two results of a kind bit-identical."""
    res = {}
    for kind, phase in (('power_sum', False), ('phase_sum', True)):
        path = L.NW_REDUCE_PARTIALS if V.psum_ok(dtype, phase, classes) else L.NW_REDUCE_ROWS
        for mb, chunks in ((11, 1), (4, 3)):
            p = make(mb)
            try:
                got, st = execute(p, x, kind, classes, chunks)
            finally:
                p.close()
            assert st['reduce_path'] == path, (kind, mb, st['reduce_path'], path)
            if kind in res:
                np.testing.assert_array_equal(got, res[kind])
            res[kind] = got
    assert res['power_sum'].dtype == np.float64 and res['phase_sum'].dtype == np.complex128
    return res


@pytest.mark.parametrize('dtype,m', SIZES)
def test_epoch_sums_every_class(dtype, m):
    """S = 11 at n = M / 2 - 1: Shannon plans (F = 1) at K = TT, TT + 1, 2 TT + 1, 4 TT + 1 with
    TT = M / 16 (variants 1, 2, 4, 8 of the E = 16 partial-sum kernels) and one Morse plan, all rows
    in class M.  NW_REDUCE_PARTIALS for fp32 M <= 8192, fp64 power at every M and fp64 phases at
    M <= 2048; NW_REDUCE_ROWS elsewhere; both against the same reference."""
    n, S = m // 2 - 1, 11
    assert V.chirp_supported(n, dtype)
    tt = m // 16
    expect = {('float32', False): m <= 8192, ('float32', True): m <= 8192, ('float64', False): True,
              ('float64', True): m <= 2048}
    for phase in (False, True):
        assert V.psum_ok(dtype, phase, [m]) == expect[dtype, phase]
    x = V.noise(S, n, 900 + m, dtype)
    supports = [tt, tt + 1, 2 * tt + 1, 4 * tt + 1]
    assert {V.chirp_class(n, k, dtype) for k in supports} == {m}
    if V.chirp_e(m, dtype, 'power_sum'):             # fp32 M = 16384 has no partial-sum kernel
        assert predict(n, supports, dtype, 'power_sum') == [(m, v) for v in (1, 2, 4, 8)]
    for k in supports:
        row = V.shannon_row(V.shannon_delta(k), n)
        assert V.table_support(row) == k
        ref = reference(x, row[None].astype(np.complex128))
        res = run_sums(lambda mb: shannon_plan(n, dtype, k, mb), x, dtype, m, [m])
        check_sums(res, ref, dtype, f'sums shannon K={k} M={m} {dtype}')
    outs = ['cwt', 'power'] + (['power_sum'] if V.chirp_e(m, dtype, 'power_sum') else [])
    freqs, pred = choose_freqs('morse', n, dtype, outs, want_classes={m}, limit=8)
    assert len(freqs) >= 4 and {c for c, _ in pred} == {m}, (freqs, pred)
    rows = analytic_rows('morse', n, freqs, False)
    ref = reference(x, rows)
    g = L.trans_grid(n / 1000., 1000., False)

    def morse(mb):
        p = nw.Plan(n, len(freqs), dtype, max_batch=mb)
        p.set_wavelet('morse', [17.5, 3.], np.array(freqs), g)
        return p
    res = run_sums(morse, x, dtype, m, [m])
    check_sums(res, ref, dtype, f'sums morse M={m} {dtype}')
