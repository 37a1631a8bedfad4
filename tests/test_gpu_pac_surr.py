"""GPU tests of the time-lag surrogate statistics of phase-amplitude coupling: nw_execute_pac_surr
(nw_pac_stage_kernel and nw_pac_surr_kernel, nw_pac_surr.hip) through Plan.execute_pac_surr,
engine.finalize_pac_surr, WaveletBase.pac_surrogates_batch and EpochsWavelet.pac_surrogates.

For epoch e, a pair (p, a), listed scales and a window of T samples as in test_gpu_pac.py, with A_j and u_j the
amplitude and the unit phasor at the window index j and a lag l in [0, T):
    M_l = sum_j A[(j + l) mod T] u[j],   all[..., s] = M_{lags[s]},   M = M_0,
    Mc = M (plain) or M - (sum u)(sum A) / T (debiased),  q = |Mc|^2,  h = |Mc|,
    stat = {sum_s h_s, sum_s q_s, #{s : q_s >= q_0}, max_s q_s}.
Inputs, plans, PAIRS, scales and windows are test_gpu_pac.py's (the coupled recipe of epoch_cases.py, E = 3, C = 5,
FREQS, phase [0 .. 3], amp [4 .. 8], max_batch = 2 C + 3); the two-pass row takes epoch_cases.SHAPES' entry and four
lags.  Lags per window: [0, 1, 63, 64, 65, T - 64, T - 1] inside [0, T), one of them repeated, then
default_rng(2700 + n).integers(lo, T - lo + 1, 32), lo = max(1, T // 10); the one-sample window takes [0], the empty
window none.

  S1  bit for bit, fp32 and fp64: M, amp, phase are execute_pac's on the same plan; all[..., s] of a lag 0 is M; a
      cell's all and stat under another pair list, other / repeated scale lists (9 x 17 scales: four partial
      tiles), another max_batch, device tensors; all[..., s] under a permuted lag list.
  S2  fp32 and fp64: the same plan's own rows restated in numpy in the contract's order (lane_sum over A_roll u):
      all within 1e-13 T A_a (test_gpu_pac.py's T2 allowance: hypot and the division may differ in the last place).
  S3  the statistics recomputed from the device's own all (and its amp and phase for the debiased centring) in the
      stated sequential order: sum q, the count and max q array_equal; sum h within 4 ulp.
  S4  against the oracle: |all - ref| <= bM_s, test_gpu_pac.py's T1 bound with the shifted amplitude,
      2 tol A_a (T + sum_j u_j) + sum_j A[(j + l)] u_j + 1e-13 T A_a.  Statistics, fp64 and the plain centring only:
      |z - z_ref| <= (2 + |z_ref|) max_s bM_s / (sd_ref - max_s bM_s), equal counts, surr_mean (mvl) within
      max_s bM_s / T -- after asserting ON THE REFERENCE ALONE that max bM / sd <= 1e-6 and that no (cell, lag) has
      |h_s - h_0| <= bM_s + bM_0 (a lag 0 of the list is the observed value itself, q_s == q_0 on the device and on the
      reference alike, and is left out of that condition).  fp32 statistics are not compared with the oracle: at tol = 1e-5 that band holds
      3 - 10 % of the comparisons and bM / sd reaches 1.4; S2 and S3 carry fp32.
      There is no assert that the planted cell's z exceeds the uncoupled cells': the 7 Hz driver of the recipe is
      strictly periodic, so a shifted surrogate keeps the coupling -- on the reference, with these lags, at n = 1024
      and n = 1201 the coupled cells have z = -0.9 .. 2.4 and the cells of the uncoupled channels reach 2.4.
  S5  the layers; S6 the debug library."""
import ctypes

import numpy as np
import pytest

from epoch_cases import (FREQS, SHAPES, FakeEpochs, forms, lane_sum, morse_plan, run_under_bounds_checks, tol_of,
                         windows_of)
from epoch_cases import coupled_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import (PAC_SURR_STATS, draw_lags, finalize_pac, finalize_pac_surr,  # noqa: E402
                                    time_window)

PHASE, AMP = [0, 1, 2, 3], [4, 5, 6, 7, 8]
FREQS26 = [float(f) for f in np.round(np.geomspace(4., 300., 26), 2)]
KINDS = ('mvl', 'mvl_norm', 'direct_pac', 'debiased_pac')
# test_gpu_pac.py's PAIRS: every channel with itself, then three cross-channel pairs
PAIRS = (np.array([0, 1, 2, 3, 4, 0, 1, 2]), np.array([0, 1, 2, 3, 4, 2, 0, 3]))
CENTRES = ('plain', 'debiased')


def pairs_of(C):
    ip, ia = PAIRS
    keep = (ip < C) & (ia < C)
    return ip[keep], ia[keep]


def lags_of(n, T, few=False):
    """The lags of a window of T samples: the edges (one repeated), then the draw; ``few``: four of the edges."""
    if T == 0:
        return np.zeros(0, dtype=np.int64)
    if T == 1:
        return np.zeros(1, dtype=np.int64)
    edge = [l for l in (0, 1, 63, 64, 65, T - 64, T - 1) if 0 <= l < T]
    if few:
        return np.array([0, 65, T - 64, T - 1], dtype=np.int64) % T
    lo = max(1, T // 10)
    draw = np.random.default_rng(2700 + n).integers(lo, T - lo + 1, 32)
    return np.concatenate([edge, edge[1:2], draw]).astype(np.int64)


def ref_all(y, ip, ia, fph, fam, idx, lags, Ac, tol):
    """The oracle's (M_l (E, P, Fp, Fa, 1 + S), bM_l likewise) over the samples ``idx`` of rows y (E, C, F, n), the lag 0
    first and then ``lags``; bM: the T1 bound of test_gpu_pac.py with the shifted amplitude."""
    yw = y[..., idx]
    T = len(idx)
    A, mp = np.abs(yw[:, :, fam]), np.abs(yw[:, :, fph])
    with np.errstate(invalid='ignore', divide='ignore'):
        u = yw[:, :, fph] / mp                                                    # (E, C, Fp, T)
        uj = np.minimum(2., 2 * tol * Ac[:, :, None, None] / mp)
    Aa = Ac[:, ia][:, :, None, None]
    fixed = 2 * tol * Aa * (T + uj.sum(-1)[:, ip][:, :, :, None]) + 1e-13 * T * Aa
    Ms, bs = [], []
    for l in [0] + list(lags):
        Al = np.roll(A, -int(l), axis=-1)[:, ia]                                  # A[(j + l) mod T]
        Ms.append(np.einsum('epit,epkt->epik', u[:, ip], Al.astype(np.complex128)))
        bs.append(fixed + np.einsum('epkt,epit->epik', Al, uj[:, ip]))
    return np.stack(Ms, axis=-1), np.stack(bs, axis=-1)


def own_all(rows, ip, ia, fph, fam, idx, lags):
    """all (E, P, Fp, Fa, S) of the plan's own complex128 rows (E, C, F, n_out) in the contract's order."""
    yw = rows[..., idx]
    re, im = np.ascontiguousarray(yw.real), np.ascontiguousarray(yw.imag)
    A = np.hypot(re[:, :, fam], im[:, :, fam])                                    # (E, C, Fa, T)
    with np.errstate(invalid='ignore', divide='ignore'):
        h = np.hypot(re[:, :, fph], im[:, :, fph])
        ur, ui = (re[:, :, fph] / h)[:, ip][:, :, :, None], (im[:, :, fph] / h)[:, ip][:, :, :, None]
    out = np.empty((rows.shape[0], len(ip), len(fph), len(fam), len(lags)), dtype=np.complex128)
    for s, l in enumerate(lags):
        Al = np.roll(A, -int(l), axis=-1)[:, ia][:, :, None]                      # (E, P, 1, Fa, T)
        out[..., s] = lane_sum(Al * ur) + 1j * lane_sum(Al * ui)
    return out


def centred(M, amp, phase, ip, ia, T, centre):
    """(re, im) of Mc for M (E, P, Fp, Fa[, S]): the device's D, each operation rounded on its own."""
    re, im = np.array(M.real), np.array(M.imag)
    if centre == 'debiased':
        P, sA = phase[:, ip][:, :, :, None], amp[:, ia][:, :, None, :, 0]
        with np.errstate(invalid='ignore', divide='ignore'):
            dre, dim = (P.real * sA) / float(T), (P.imag * sA) / float(T)
        if M.ndim == 5:
            dre, dim = dre[..., None], dim[..., None]
        re, im = re - dre, im - dim
    return re, im


def stats_of(M, amp, phase, all_, ip, ia, T, centre):
    """stat (E, P, Fp, Fa, 4) from the sums, in the contract's sequential order over the lag list."""
    r0, i0 = centred(M, amp, phase, ip, ia, T, centre)
    q0 = r0 * r0 + i0 * i0
    rs, is_ = centred(all_, amp, phase, ip, ia, T, centre)
    sh, sq, cnt, mx = (np.zeros(M.shape) for _ in range(4))
    for s in range(all_.shape[-1]):
        q = rs[..., s] * rs[..., s] + is_[..., s] * is_[..., s]
        sh, sq = sh + np.sqrt(q), sq + q
        with np.errstate(invalid='ignore'):
            cnt = cnt + (q >= q0)
            mx = np.where(q > mx, q, mx)
    return np.stack([sh, sq, cnt, mx], axis=-1)


def check_s3(name, sums, ip, ia, T, centre):
    M, amp, phase, stat, all_ = sums
    want = stats_of(M, amp, phase, all_, ip, ia, T, centre)
    dh = np.abs(stat[..., 0] - want[..., 0]) / np.spacing(np.abs(want[..., 0]))
    print(f'{name} {centre} S3: sum q, count, max q compared bit for bit; sum h differs by {np.max(dh, initial=0.):.0f} ulp at most')
    for k, what in ((1, 'sum q'), (2, 'count'), (3, 'max q')):
        assert np.array_equal(stat[..., k], want[..., k]), (name, centre, what)
    assert np.all(dh <= 4), (name, centre, dh.max())


# (id, n, dtype, E, C, freqs, phase, amp, plan keywords, device decim, host decim, four lags only)
CASES = []
for name, n, dtype, kw, decim, host_decim, _ in forms('1024-f32', '1024-f64', 'chirp-1201-f32', 'chirp-1201-f64',
                                                      'decim-4096', 'rocfft-1000-step4', 'twopass-32768'):
    if name in SHAPES:
        E, C, freqs = SHAPES[name]
        CASES.append((name, n, dtype, E, C, freqs, [0], [1, 2], kw, decim, host_decim, True))
    else:
        CASES.append((name, n, dtype, 3, 5, FREQS, PHASE, AMP, kw, decim, host_decim, False))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_surrogates_against_execute_pac_the_plans_own_rows_and_the_oracle(case):
    """S1 (execute_pac's sums, the lag 0), S2, S3 and S4 for every form and window, both centrings."""
    name, n, dtype, E, C, freqs, fph, fam, kw, decim, host_decim, few = case
    x, y = oracle_rows(n, E, C, dtype, freqs)
    Ac = np.max(np.abs(y), axis=(2, 3))                       # (E, C), of the undecimated rows
    ip, ia = pairs_of(C)
    tol = tol_of(n, dtype)
    n_out = n // decim
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        got = {}
        for wname, win, step in windows_of(n, n_out, host_decim):
            T = len(range(win[0], win[1], step))
            lags = lags_of(n, T, few)
            pac = p.execute_pac(x, (ip, ia), fph, fam, win, step)
            sur = {c: p.execute_pac_surr(x, lags, (ip, ia), fph, fam, win, step, centre=c, keep_all=True) for c in CENTRES}
            st = p.stats()
            assert st['reduce_path'] == L.NW_REDUCE_PAC_SURR, (name, st)
            got[wname] = (win, step, lags, pac, sur)
        rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, len(freqs), n_out)
    finally:
        p.close()
    for wname, (win, step, lags, pac, sur) in got.items():
        tag = f'{name} {wname}'
        idx = np.arange(win[0], win[1], step)
        T, S = len(idx), len(lags)
        shape = (E, len(ip), len(fph), len(fam))
        for c in CENTRES:
            M, amp, phase, stat, all_ = sur[c]
            assert stat.dtype == np.float64 and stat.shape == shape + (4,), tag
            assert all_.dtype == np.complex128 and all_.shape == shape + (S,), tag
            for u, v in zip((M, amp, phase), pac):                                 # S1
                assert u.dtype == v.dtype and np.array_equal(u, v), (tag, c)
            for s in np.flatnonzero(lags == 0):
                assert np.array_equal(all_[..., s], M), (tag, c, s)
            assert np.array_equal(all_, sur['plain'][4]), (tag, c)                 # all is M, not Mc
            if T == 0:                                             # an empty window: zero sums, no lags
                assert S == 0 and not np.any(M) and not np.any(stat), tag
                continue
            assert np.all(np.isfinite(stat)) and np.all(np.isfinite(all_.view(np.float64))), (tag, c)
            check_s3(tag, sur[c], ip, ia, T, c)                                    # S3
        if T == 0:
            continue
        M, amp, phase, stat, all_ = sur['plain']
        # S2: the plan's own rows in the contract's order
        d2 = np.abs(all_ - own_all(rows, ip, ia, fph, fam, idx, lags)) / Ac[:, ia][:, :, None, None, None]
        print(f'{tag} S2: all within {d2.max():.2e} A_a of the own rows in numpy (bound {1e-13 * T:.1e})')
        assert d2.max() <= 1e-13 * T, (tag, d2.max())
        # S4: the oracle
        rM, bM = ref_all(y, ip, ia, fph, fam, idx * decim, lags, Ac, tol)
        dM = np.abs(np.concatenate([M[..., None], all_], axis=-1) - rM)
        print(f'{tag} S4: all within {np.max(dM / bM):.3f} of its bound (tol {tol:.0e})')
        assert np.all(dM <= bM), (tag, np.max(dM / bM))
        if dtype != 'float64' or S < 2:
            continue
        rh = np.abs(rM)
        h0, hs, b0, bs = rh[..., 0], rh[..., 1:], bM[..., 0], bM[..., 1:]
        mean_ref, sd_ref = hs.mean(-1), hs.std(-1)
        bmax = bM.max(-1)
        # on the reference alone
        band = np.abs(hs - h0[..., None]) <= bs + b0[..., None]
        band[..., lags == 0] = False                               # the lag 0 is the observed value itself: q_s == q_0
        print(f'{tag} S4 reference: max bM / sd {np.max(bmax / sd_ref):.2e}, {np.count_nonzero(band)} (cell, lag) in the band')
        assert np.max(bmax / sd_ref) <= 1e-6, (tag, np.max(bmax / sd_ref))
        assert not np.any(band), (tag, np.count_nonzero(band))
        z_ref = (h0 - mean_ref) / sd_ref
        z = finalize_pac_surr('mvl', 'zscore', M, amp, phase, stat, None, ip, ia, T, S)
        zb = (2 + np.abs(z_ref)) * bmax / (sd_ref - bmax)
        print(f'{tag} S4: z within {np.max(np.abs(z - z_ref) / zb):.3f} of its bound; z_ref {z_ref.min():.2f} .. {z_ref.max():.2f}')
        assert np.all(np.abs(z - z_ref) <= zb), (tag, np.max(np.abs(z - z_ref) / zb))
        assert np.array_equal(stat[..., 2], (hs >= h0[..., None]).sum(-1)), tag
        mean = finalize_pac_surr('mvl', 'surr_mean', M, amp, phase, stat, None, ip, ia, T, S)
        assert np.all(np.abs(mean - mean_ref / T) <= bmax / T), tag


def _same_cells(a, b, what):
    for u, v, nm in zip(a[3:], b[3:], ('stat', 'all')):
        assert np.array_equal(u, v, equal_nan=True), (what, nm)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_a_cells_values_depend_only_on_its_rows_the_window_and_the_lags(dtype):
    """S1, bit for bit: any pair list, any scale lists, any chunking, device tensors, a permuted lag list."""
    import torch
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ip, ia = pairs_of(C)
    win = (37, 1001)
    T = win[1] - win[0]
    lags = lags_of(n, T)
    S = len(lags)
    la, lb = np.array([4, 0, 3, 2, 2, 0, 1]), np.array([4, 2, 3, 3, 3, 2, 0])      # shuffled, repeated, cross, own
    sph, sam = [3, 1, 1, 5, 0], [5, 8, 4, 4, 1, 6, 7]            # reordered, repeated, 5 and 1 in both lists
    perm = np.random.default_rng(7).permutation(S)
    for centre in CENTRES:
        res = {}
        for mb in (C, 2 * C + 3, E * C):
            p = morse_plan(n, dtype, FREQS, mb)
            try:
                res[mb] = p.execute_pac_surr(x, lags, (ip, ia), PHASE, AMP, win, centre=centre, keep_all=True)
                assert p.stats()['chunks'] == -(-E // (mb // C))
                if mb != 2 * C + 3:
                    continue
                lst = p.execute_pac_surr(x, lags, (la, lb), PHASE, AMP, win, centre=centre, keep_all=True)
                scl = p.execute_pac_surr(x, lags, (ip, ia), sph, sam, win, centre=centre, keep_all=True)
                prm = p.execute_pac_surr(x, lags[perm], (ip, ia), PHASE, AMP, win, centre=centre, keep_all=True)
                short = p.execute_pac_surr(x, lags, (ip, ia), PHASE, AMP, win, centre=centre)
                tx = torch.from_numpy(np.array(x)).cuda()
                P, Fp, Fa = len(ip), len(PHASE), len(AMP)
                tout = (torch.full((E, P, Fp, Fa), float('nan'), dtype=torch.complex128, device='cuda'), None, None,
                        torch.full((E, P, Fp, Fa, 4), float('nan'), dtype=torch.float64, device='cuda'),
                        torch.full((E, P, Fp, Fa, S), float('nan'), dtype=torch.complex128, device='cuda'))
                back = p.execute_pac_surr(tx, lags, (ip, ia), PHASE, AMP, win, centre=centre, keep_all=True, out=tout)
                assert back is tout
                dev = [None if t is None else t.cpu().numpy() for t in tout]
            finally:
                p.close()
        base = res[2 * C + 3]
        M, amp, phase, stat, all_ = base
        for mb in (C, E * C):                                         # any chunking
            for u, v in zip(res[mb], base):
                assert np.array_equal(u, v), (centre, mb)
        # device tensors, without the per-channel outputs (the debiased centring still has its sums)
        assert np.array_equal(dev[0], M) and np.array_equal(dev[3], stat) and np.array_equal(dev[4], all_), centre
        # keep_all=False: four results, the same statistics
        assert len(short) == 4 and np.array_equal(short[3], stat) and np.array_equal(short[0], M)
        # any pair list
        for k, (a, b) in enumerate(zip(la, lb)):
            q = int(np.flatnonzero((ip == a) & (ia == b))[0])
            assert np.array_equal(lst[3][:, k], stat[:, q]) and np.array_equal(lst[4][:, k], all_[:, q]), (centre, a, b)
        # any scale lists: a cell is its (phase scale, amplitude scale)'s, wherever it stands
        for i, fp in enumerate(sph):
            for k, fa in enumerate(sam):
                if fp in PHASE and fa in AMP:
                    at = (slice(None), slice(None), PHASE.index(fp), AMP.index(fa))
                    assert np.array_equal(scl[3][:, :, i, k], stat[at]) and np.array_equal(scl[4][:, :, i, k], all_[at]), (fp, fa)
        assert np.array_equal(scl[3][:, :, 1], scl[3][:, :, 2]) and np.array_equal(scl[4][:, :, :, 2], scl[4][:, :, :, 3])
        # a permuted lag list: every surrogate is its own lag's; the order-free statistics do not move
        assert np.array_equal(prm[4], all_[..., perm]), centre
        assert np.array_equal(prm[3][..., 2:], stat[..., 2:]), centre


def test_partial_scale_tiles():
    """S1 on 9 phase x 17 amplitude scales of FREQS26 (two phase and two amplitude tiles, one of each partial): a
    cell's values are those of the reversed lists, where it stands in another tile, wave and lane."""
    n, E, C, dtype = 1024, 2, 2, 'float64'
    x, _ = oracle_rows(n, E, C, dtype, FREQS26)
    ph, am = list(range(9)), list(range(9, 26))
    win = (37, 1001)
    lags = lags_of(n, win[1] - win[0])
    p = morse_plan(n, dtype, FREQS26, 2 * C + 3)
    try:
        for centre in CENTRES:
            a = p.execute_pac_surr(x, lags, ([0, 1, 0], [0, 1, 1]), ph, am, win, centre=centre, keep_all=True)
            b = p.execute_pac_surr(x, lags, ([0, 1, 0], [0, 1, 1]), ph[::-1], am[::-1], win, centre=centre, keep_all=True)
            one = p.execute_pac_surr(x, lags, ([0], [1]), ph[8:], am[16:], win, centre=centre, keep_all=True)
            pac = p.execute_pac(x, ([0, 1, 0], [0, 1, 1]), ph, am, win)
            assert np.array_equal(a[0], pac[0]) and np.array_equal(a[1], pac[1]) and np.array_equal(a[2], pac[2])
            assert np.all(np.isfinite(a[3]))
            assert np.array_equal(b[3][:, :, ::-1, ::-1], a[3]) and np.array_equal(b[4][:, :, ::-1, ::-1], a[4]), centre
            assert np.array_equal(one[3][:, 0, 0, 0], a[3][:, 2, 8, 16]) and np.array_equal(one[4][:, 0, 0, 0], a[4][:, 2, 8, 16])
            check_s3('tiles-9x17-f64', a, np.array([0, 1, 0]), np.array([0, 1, 1]), win[1] - win[0], centre)
    finally:
        p.close()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_edge_cases_and_errors(dtype):
    """S5: the empty window, no lags, no epochs, no pairs; a zero phase sample; the C ABI's own checks; the plan
    still works afterwards."""
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ip, ia = pairs_of(C)
    P, Fp, Fa = len(ip), len(PHASE), len(AMP)
    win = (37, 1001)
    lags = lags_of(n, win[1] - win[0])
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        host = p.execute_pac_surr(x, lags, (ip, ia), PHASE, AMP, win, keep_all=True)
        pac = p.execute_pac(x, (ip, ia), PHASE, AMP, win)
        # an empty window takes no lag: zero sums
        z = p.execute_pac_surr(x, [], (ip, ia), PHASE, AMP, (n, n), keep_all=True)
        assert len(z) == 5 and z[3].shape == (E, P, Fp, Fa, 4) and z[4].shape == (E, P, Fp, Fa, 0)
        assert not any(np.any(a) for a in z)
        with pytest.raises(ValueError, match='lags'):
            p.execute_pac_surr(x, [0], (ip, ia), PHASE, AMP, (n, n))
        # no lags: M, amp, phase and zero statistics
        z = p.execute_pac_surr(x, [], (ip, ia), PHASE, AMP, win, centre='debiased', keep_all=True)
        for u, v in zip(z[:3], pac):
            assert np.array_equal(u, v)
        assert not np.any(z[3]) and z[4].shape == (E, P, Fp, Fa, 0)
        # no epochs, no pairs: empty outputs, the per-channel sums still formed
        z = p.execute_pac_surr(x[:0], lags, (ip, ia), PHASE, AMP, win, keep_all=True)
        assert z[0].shape == (0, P, Fp, Fa) and z[3].shape == (0, P, Fp, Fa, 4) and z[4].shape == (0, P, Fp, Fa, len(lags))
        z = p.execute_pac_surr(x, lags, ([], []), PHASE, AMP, win)
        assert z[0].shape == (E, 0, Fp, Fa) and z[3].shape == (E, 0, Fp, Fa, 4)
        assert np.array_equal(z[1], pac[1]) and np.array_equal(z[2], pac[2])
        assert p.stats()['reduce_path'] == L.NW_REDUCE_PAC_SURR
        # a phase row with |y| = 0 (a zero epoch): its cells' sums are NaN and their counts 0
        xz = np.array(x)
        xz[1, 2] = 0
        z = p.execute_pac_surr(xz, lags, (ip, ia), PHASE, AMP, win)
        bad = ip == 2
        assert np.all(np.isnan(z[3][1][bad][..., :2])) and not np.any(z[3][1][bad][..., 2:])
        assert np.all(np.isfinite(z[3][0])) and np.all(np.isfinite(z[3][1][~bad & (ia != 2)]))
        # the C ABI's own checks: the message names the value
        V_ = ctypes.c_void_p
        xc = np.ascontiguousarray(x)
        ii, ff, fa_ = ip.astype(np.int32), np.array(PHASE, dtype=np.int32), np.array(AMP, dtype=np.int32)
        bufM = np.empty((E, P, Fp, Fa), dtype=np.complex128)
        bufS = np.empty((E, P, Fp, Fa, 4))

        def call(lg, nl, centre, stat, t0=37, t1=1001):
            lg = np.asarray(lg, dtype=np.int64)
            return L.lib().nw_execute_pac_surr(p.handle, xc.ctypes.data_as(V_), E, C, ii.ctypes.data_as(V_),
                                               ii.ctypes.data_as(V_), len(ii), ff.ctypes.data_as(V_), Fp,
                                               fa_.ctypes.data_as(V_), Fa, t0, t1, 1, lg.ctypes.data_as(V_), nl, centre,
                                               bufM.ctypes.data_as(V_), None, None, stat, None, L.NW_MEM_HOST)
        for args, word in ((([5, 964], 2, 0, bufS.ctypes.data_as(V_)), b'lag 1 = 964'),
                           (([5, -1], 2, 0, bufS.ctypes.data_as(V_)), b'lag 1 = -1'),
                           (([0], 1, 0, bufS.ctypes.data_as(V_), 500, 500), b'lag 0 = 0'),
                           (([5], -1, 0, bufS.ctypes.data_as(V_)), b'nlags (-1)'),
                           (([5], L.NW_PAC_MAX_LAGS + 1, 0, bufS.ctypes.data_as(V_)), b'nlags (4097)'),
                           (([5], 1, 2, bufS.ctypes.data_as(V_)), b'centre'),
                           (([5], 1, 0, None), b'null argument')):
            rc = call(*args)
            assert rc == L.NW_E_INVALID and word in L.lib().nw_last_error(), (args[:3], L.lib().nw_last_error())
        assert call([5, 963], 2, 1, bufS.ctypes.data_as(V_)) == L.NW_OK
        small = morse_plan(n, dtype, FREQS, C - 1)
        try:
            with pytest.raises(ValueError, match='max_batch'):
                small.execute_pac_surr(x, lags, None, PHASE, AMP)
        finally:
            small.close()
        # the staged rows are the plan's: counted, and the plan still works
        assert p.stats()['device_bytes'] >= 2 * C * (2 * Fp + Fa) * (win[1] - win[0]) * 8
        again = p.execute_pac_surr(x, lags, (ip, ia), PHASE, AMP, win, keep_all=True)
        for u, v in zip(again, host):
            assert np.array_equal(u, v)
        for u, v in zip(p.execute_pac(x, (ip, ia), PHASE, AMP, win), pac):
            assert np.array_equal(u, v)
        assert p.stats()['reduce_path'] == L.NW_REDUCE_PAC
    finally:
        p.close()


def test_class_layer():
    """S5: pac_surrogates_batch is finalize_pac_surr of Plan.execute_pac_surr for every out x stat, with device
    decim; average; the seeded draw; EpochsWavelet.pac_surrogates' concatenated scale list and padding."""
    E, C = 3, 5
    own = np.arange(C)
    cross = (np.array([0, 2, 1]), np.array([2, 1, 1]))
    n, dtype = 4096, 'float32'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype)
    win = (150, 4001)
    t0, t1, step, T = time_window(n, 4, win, True)
    assert (t0, t1, step, T) == (38, 1001, 1, 963)
    lags = lags_of(n, T)[:16]
    S = len(lags)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, decim=4)
    try:
        sums = {c: p.execute_pac_surr(x, lags, None, PHASE, AMP, (t0, t1), step, centre=c, keep_all=True) for c in CENTRES}
        csums = p.execute_pac_surr(x, lags, cross, PHASE, AMP, (t0, t1), step, keep_all=True)
        drawn = p.execute_pac_surr(x, draw_lags(T, 24, seed=5), None, PHASE, AMP, (t0, t1), step)
    finally:
        p.close()
    kw = dict(phase=PHASE, amp=AMP, window=win, decim=4)
    for out in KINDS:
        s5 = sums['debiased' if out == 'debiased_pac' else 'plain']
        for stat in sorted(PAC_SURR_STATS - {'surr_sum'}):
            want = finalize_pac_surr(out, stat, *s5, own, own, T, S)
            got = w.pac_surrogates_batch(x, FREQS, out=out, stat=stat, lags=lags, **kw)
            assert got.shape == (E, C, len(PHASE), len(AMP)) + ((S,) if stat == 'surrogates' else ()), (out, stat)
            assert np.array_equal(got, want, equal_nan=True), (out, stat)
            if stat in ('zscore', 'surr_mean', 'surr_std'):
                avg = w.pac_surrogates_batch(x, FREQS, out=out, stat=stat, lags=lags, average=True, **kw)
                assert avg.shape == (C, len(PHASE), len(AMP)) and np.array_equal(avg, want.mean(axis=0)), (out, stat)
        # the observed value of the surrogates' measure is finalize_pac's: the lag 0 among the surrogates
        vals = finalize_pac_surr(out, 'surrogates', *s5, own, own, T, S)
        obs = finalize_pac(out, *s5[:3], own, own, T)
        assert np.allclose(vals[..., int(np.flatnonzero(lags == 0)[0])], obs, rtol=1e-12, atol=0), out
    got = w.pac_surrogates_batch(x, FREQS, stat='surr_sum', lags=lags, **kw)
    assert len(got) == 5 and got[4] is None
    for u, v in zip(got[:4], sums['plain']):
        assert np.array_equal(u, v)
    got = w.pac_surrogates_batch(x, FREQS, stat='pvalue', lags=lags, indices=cross, **kw)
    assert np.array_equal(got, finalize_pac_surr('direct_pac', 'pvalue', *csums, *cross, T, S))
    assert got.min() >= 1 / (1 + S) and got.max() <= 1
    # the draw: lags=None is default_rng(seed).integers(min_lag, T - min_lag + 1, n_surrogates), reproducible
    a = w.pac_surrogates_batch(x, FREQS, n_surrogates=24, seed=5, **kw)
    assert np.array_equal(a, finalize_pac_surr('direct_pac', 'zscore', *drawn, None, own, own, T, 24))
    assert np.array_equal(a, w.pac_surrogates_batch(x, FREQS, n_surrogates=24, seed=5, **kw))
    assert not np.array_equal(a, w.pac_surrogates_batch(x, FREQS, n_surrogates=24, seed=6, **kw))
    assert w.pac_surrogates_batch(x, FREQS, phase=PHASE, amp=AMP, n_surrogates=8, seed=1).shape == (E, C, len(PHASE), len(AMP))
    assert w.plan_stats()[-1]['reduce_path'] == L.NW_REDUCE_PAC_SURR
    # EpochsWavelet: the two frequency lists concatenated, padding in seconds, channels picked by name
    n, dtype = 1000, 'float64'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype, engine='rocfft')
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)                 # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype, engine='rocfft'))
    sub = np.ascontiguousarray(x[:, :3])
    pf, af = [FREQS[i] for i in PHASE], [FREQS[i] for i in AMP]
    idx = ([2, 0], [0, 1])
    for method, stat in (('direct_pac', 'zscore'), ('debiased_pac', 'pvalue'), ('mvl_norm', 'surr_max')):
        assert np.array_equal(ew.pac_surrogates(['a', 'b', 'c'], pf, af, method=method, stat=stat, n_surrogates=12, seed=3,
                                                padding=0.0371),
                              w.pac_surrogates_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, stat=stat, n_surrogates=12,
                                                     seed=3, window=(37, n - 37))), (method, stat)
    assert np.array_equal(ew.pac_surrogates(['a', 'b', 'c'], pf, af, lags=[3, 100, 7], indices=idx, padding=0.1, decim=4,
                                            average=True),
                          w.pac_surrogates_batch(sub, FREQS, phase=PHASE, amp=AMP, lags=[3, 100, 7], indices=idx,
                                                 window=(100, 900), decim=4, average=True))
    with pytest.raises(ValueError, match='padding'):
        ew.pac_surrogates(['a', 'b'], pf, af, padding=0.5)


def test_pac_surr_under_bounds_checks():
    """S6: the debug library (kernel bounds checks, nw_dcheck.h) on the chirp-z length 1201 (a tail tile), the window
    (37, 1001) and a strided one, the edge lags, both centrings, own and cross-channel pairs, partial tiles: no
    check fails."""
    body = ('rng = np.random.default_rng(1)\n'
            'n, E, C, F = 1201, 3, 5, 9\n'
            'x = rng.standard_normal((E, C, n))\n'
            'p = nw.Plan(n, F, "float64", max_batch=2 * C + 3)\n'
            'p.set_wavelet("morse", [17.5, 3.], np.geomspace(3., 300., F), L.trans_grid(n / 1000., 1000., False))\n'
            'ok = True\n'
            'for win, step in (((37, 1001), 1), ((5, n), 4), ((0, 1), 1), ((9, 9), 1)):\n'
            '    T = len(range(win[0], win[1], step))\n'
            '    lags = sorted({l for l in (0, 1, 63, 64, 65, T - 64, T - 1) if 0 <= l < T})\n'
            '    for centre in ("plain", "debiased"):\n'
            '        own = p.execute_pac_surr(x, lags, None, [0, 1, 2, 3], [4, 5, 6, 7, 8], win, step, centre=centre, keep_all=True)\n'
            '        short = p.execute_pac_surr(x, lags + lags[:1], ([C - 1, 0, 1], [0, 0, 1]), list(range(9)), list(range(9)) * 2, win, step, centre=centre)\n'
            '        for a in own + short:\n'
            '            ok = ok and bool(np.all(np.isfinite(a))) and a.shape[0] == E\n'
            'print("ok", ok)\n'
            'p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok True' in lines, lines
