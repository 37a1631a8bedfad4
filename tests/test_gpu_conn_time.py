"""GPU tests of over-time connectivity: nw_execute_conn_time (nw_conn_time_kernel and
nw_conn_time_power_kernel, nw_conn_time.hip) through Plan.execute_conn_time, engine.finalize_conn_time,
WaveletBase.connectivity_time_batch and EpochsWavelet.connectivity_time.

For epoch e, channels c with rows y_e,c (F, n_out), a pair (a, b), a window of T samples s_j = t0 + j step
and m_j = Im y_a conj(y_b) at s_j:
    S = sum_j y_a conj(y_b),  P_cc = sum_j |y_c|^2,  Phi = sum_j (y_a / |y_a|) conj(y_b / |y_b|),
    L0 .. L3 = sum_j of m_j, |m_j|, m_j^2, sgn m_j
one value per (e, pair, f).  References are formed here from oracle.nw_oracle in complex128.

Inputs: the lagged recipe of epoch_cases.py: rng = default_rng(2300 + n), x[:, c] = 0.6 roll(common, 3 c) +
0.8 noise[:, c]; Morse(1000) with its default b, r and the nine scales FREQS (three, FREQS3, where stated).
E = 3 epochs and C = 5 channels unless stated; max_batch = 2 C + 3: chunks of 2 and 1 epochs.
Windows (in the plan's output samples): full, (0, 1), (37, 1001) and an empty one; the full-rate n = 1000 plan
of the rocFFT case takes them through engine.time_window with decim = 4 (its step-4 path), where (37, 1001)
is cut to the signal's end: (40, 1000) step 4.

tol: 1e-12 fp64, 1e-5 fp32, 2e-5 fp32 on chirp-z lengths (the per-signal contract); A_e,c: that signal's
max |y| over (F, N) of the undecimated rows.
  T1  against the oracle: |dS|, |dL0|, |dL1| <= 2 tol T A_a A_b; |dP_cc| <= 2 tol T A_c^2; |dL2| <= 5 tol T
      (A_a A_b)^2; |dPhi| <= sum_j min(2, u_a + u_b + u_a u_b) + 1e-13 T with u_c = 2 tol A_c / |y_c| (a unit
      phasor moves by at most 2 |dy| / |y|); |dL3| <= 2 K, K = the window samples at which the reference has
      |m| < v A_a A_b, v = 1e-4 fp32 / 1e-9 fp64 (only those can flip a sign).  On the reference alone, for the
      windows of more than one sample: sum min(..) <= 0.02 T; K <= 0.7 T (fp32); K = 0 everywhere (fp64).
  T2  fp64, bit for bit: the same plan's own rows reduced in numpy in the contract's order (lane sums in j
      order, then the halving fold, every product and term a separate numpy operation): S, P_cc and the four lag
      sums array_equal, Phi within 1e-13 T (hypot and the division may differ in the last place).
  T3  fp64 identities, bit for bit: L0 == Im S; a pair's sums under any index list; any chunking; device tensors.
  T4  measures: fp64 every finalised kind within 1e-7 of the same formula on the oracle's sums; fp32
      |dwpli| <= 4 tol / (L1 / (T A_a A_b) - 2 tol) and |dcoherence| <= 4 tol / (sqrt(P_aa P_bb) / (T A_a A_b) -
      2 tol) where that bound is <= 0.05: at least 0.7 (wpli) / 0.85 (coherence) of every pair's (e, f), asserted
      on the reference alone; pli and dpli from the L3 bound.
  T5  the layers; T6 the debug library."""
import numpy as np
import pytest

from epoch_cases import (FREQS, FREQS3, OVER_TIME, SHAPES, FakeEpochs, forms, lane_sum, morse_plan,
                         run_under_bounds_checks, tol_of, vis_of, windows_of)
from epoch_cases import lagged_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import (CONN_OUTS, LAG_OUTS, all_pairs, finalize_conn_time, finalize_lag,  # noqa: E402
                                    finalize_pair, time_window)

KINDS = ('cross_sum', 'plv_sum', 'lag_sum')
MEASURES = [k for k in list(CONN_OUTS) + list(LAG_OUTS) if not k.endswith('_sum')]


def run_all(p, x, indices, win, step):
    """The three kinds of sums of one window: (S, P, Phi, lag)."""
    S, P = p.execute_conn_time(x, indices, win, step, out_kind='cross_sum')
    phi = p.execute_conn_time(x, indices, win, step, out_kind='plv_sum')
    lag = p.execute_conn_time(x, indices, win, step, out_kind='lag_sum')
    return S, P, phi, lag


def ref_sums(y, ia, ib, idx):
    """The oracle's sums over the samples ``idx`` of rows y (E, C, F, n): (S (E, P, F), P (E, C, F),
    Phi (E, P, F), lag (E, P, F, 4), m (E, P, F, T), a, b)."""
    yw = y[..., idx]
    a, b = yw[:, ia], yw[:, ib]
    prod = a * np.conj(b)
    with np.errstate(invalid='ignore', divide='ignore'):
        phi = np.sum(a / np.abs(a) * np.conj(b / np.abs(b)), axis=-1)
    m = prod.imag
    lag = np.stack([m.sum(-1), np.abs(m).sum(-1), (m * m).sum(-1), np.sign(m).sum(-1)], axis=-1)
    return prod.sum(-1), np.sum(yw.real ** 2 + yw.imag ** 2, axis=-1), phi, lag, m, a, b


def check_t1(name, got, y, A, ia, ib, idx, tol, dtype, listed=True):
    """T1 of (S, P, Phi, lag) over the window samples ``idx`` (indices into the reference rows)."""
    S, P, phi, lag = got
    T = len(idx)
    rS, rP, rphi, rlag, m, a, b = ref_sums(y, ia, ib, idx)
    AB = (A[:, ia] * A[:, ib])[:, :, None]                                       # (E, P, 1)
    with np.errstate(divide='ignore'):
        ua = 2 * tol * A[:, ia][:, :, None, None] / np.abs(a)
        ub = 2 * tol * A[:, ib][:, :, None, None] / np.abs(b)
    bphi = np.sum(np.minimum(2., ua + ub + ua * ub), axis=-1)
    K = np.sum(np.abs(m) < vis_of(dtype) * AB[..., None], axis=-1)
    # on the reference alone
    if T > 1 and listed:
        assert np.all(bphi <= 0.02 * T), (name, bphi.max() / T)
        if dtype == 'float64':
            assert not np.any(K), (name, K.max())
        else:
            assert np.all(K <= 0.7 * T), (name, K.max() / T)
    print(f'{name} T={T}: reference: phasor bound <= {bphi.max() / max(T, 1):.4f} T, K <= {K.max() / max(T, 1):.3f} T')
    scale = max(T, 1)
    dS = np.abs(S - rS) / (AB * scale)
    dP = np.abs(P - rP) / (A[:, :, None] ** 2 * scale)
    d = np.abs(lag - rlag)
    d0, d1, d2 = d[..., 0] / (AB * scale), d[..., 1] / (AB * scale), d[..., 2] / (AB ** 2 * scale)
    dphi = np.abs(phi - rphi)
    print(f'{name} T1: dS {dS.max() / (2 * tol):.3f} dP {dP.max() / (2 * tol):.3f} dL0 {d0.max() / (2 * tol):.3f} '
          f'dL1 {d1.max() / (2 * tol):.3f} dL2 {d2.max() / (5 * tol):.3f} of the bound (tol {tol:.0e}); dPhi '
          f'{np.max(dphi - bphi - 1e-13 * T):.3e} over its bound; dL3 {np.max(d[..., 3] - 2 * K):.0f} over 2K')
    assert S.shape == rS.shape and P.shape == rP.shape and phi.shape == rphi.shape and lag.shape == rlag.shape
    assert dS.max() <= 2 * tol and dP.max() <= 2 * tol, (name, dS.max(), dP.max())
    assert d0.max() <= 2 * tol and d1.max() <= 2 * tol and d2.max() <= 5 * tol, (name, d0.max(), d1.max(), d2.max())
    assert np.all(dphi <= bphi + 1e-13 * T), name
    assert np.all(d[..., 3] <= 2 * K), name
    assert np.array_equal(lag[..., 3], np.rint(lag[..., 3])), name                # L3 holds integers
    return rS, rP, rphi, rlag, K


def own_sums(rows, ia, ib, idx):
    """(S, P, Phi, lag) of the plan's own complex128 rows (E, C, F, n_out) in the contract's order."""
    yw = rows[..., idx]
    re, im = np.ascontiguousarray(yw.real), np.ascontiguousarray(yw.imag)
    ar, ai, br, bi = re[:, ia], im[:, ia], re[:, ib], im[:, ib]
    t1, t2 = ar * br, ai * bi
    t3, t4 = ai * br, ar * bi
    m = t3 + (-t4)
    S = lane_sum(t1 + t2) + 1j * lane_sum(m)
    p1, p2 = re * re, im * im
    P = lane_sum(p1 + p2)
    lag = np.stack([lane_sum(m), lane_sum(np.abs(m)), lane_sum(m * m), lane_sum(np.sign(m))], axis=-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        mag = np.hypot(re, im)
        ur, ui = re / mag, im / mag
    uar, uai, ubr, ubi = ur[:, ia], ui[:, ia], ur[:, ib], ui[:, ib]
    q1, q2, q3, q4 = uar * ubr, uai * ubi, uai * ubr, uar * ubi
    phi = lane_sum(q1 + q2) + 1j * lane_sum(q3 + (-q4))
    return S, P, phi, lag


# (id, n, dtype, E, C, freqs, plan keywords, device decim, host decim, kernel of the form): three epochs but for the
# rows of SHAPES
CASES = []
for name, n, dtype, kw, decim, host_decim, kernel in forms(*OVER_TIME):
    E, C, freqs = SHAPES.get(name, (3, 5, FREQS))
    CASES.append((name, n, dtype, E, C, freqs, kw, decim, host_decim, kernel))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 for every case and window, T2 for the fp64 cases; every pair a < b; max_batch = 2 C + 3."""
    name, n, dtype, E, C, freqs, kw, decim, host_decim, kernel = case
    x, y = oracle_rows(n, E, C, dtype, freqs)
    A = np.max(np.abs(y), axis=(2, 3))                        # (E, C), of the undecimated rows
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    n_out = n // decim
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        assert p.n_out == n_out
        got = {}
        for wname, win, step in windows_of(n, n_out, host_decim):
            got[wname] = (win, step, run_all(p, x, None, win, step))
            st = p.stats()
            assert st['reduce_path'] == L.NW_REDUCE_CONN_TIME and L.KERNEL_NAMES[st['kernel']] == kernel, (name, st)
        assert st['chunks'] == 3 * len(got) * -(-E // 2), (name, st)
        rows = None
        if dtype == 'float64':
            rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, len(freqs), n_out)
    finally:
        p.close()
    if C > 16:
        assert L.conn_tiles(C, ia, ib)[1] == 3
    for wname, (win, step, sums) in got.items():
        idx = np.arange(win[0], win[1], step)
        assert len(idx) == L.conn_time_count(n_out, win[0], win[1], step)
        S, P, phi, lag = sums
        assert S.dtype == np.complex128 and P.dtype == np.float64 and phi.dtype == np.complex128 and lag.dtype == np.float64
        assert S.shape == (E, len(ia), len(freqs)) and P.shape == (E, C, len(freqs)) and lag.shape == S.shape + (4,)
        if len(idx) == 0:                                      # an empty window: zero sums
            assert not np.any(S) and not np.any(P) and not np.any(phi) and not np.any(lag), (name, wname)
            continue
        check_t1(f'{name} {wname}', sums, y, A, ia, ib, idx * decim, tol, dtype, wname != 'stride')
        if rows is not None:                                   # T2
            oS, oP, ophi, olag = own_sums(rows, ia, ib, idx)
            assert np.array_equal(S, oS) and np.array_equal(P, oP), (name, wname, np.abs(S - oS).max())
            assert np.array_equal(lag, olag), (name, wname, [np.abs(lag - olag)[..., k].max() for k in range(4)])
            dphi = np.abs(phi - ophi).max()
            print(f'{name} {wname} T2: S, P and the lag sums equal bit for bit; dPhi {dphi:.2e} (bound {1e-13 * len(idx):.1e})')
            assert dphi <= 1e-13 * len(idx), (name, wname, dphi)
            assert np.array_equal(lag[..., 0], S.imag), (name, wname)          # T3: L0 == Im S


def test_a_pairs_sums_do_not_depend_on_the_list_the_tiling_or_the_chunks():
    """T3, fp64, bit for bit."""
    n, dtype, E, C = 1024, 'float64', 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    la = np.array([4, 0, 3, 3, 0, 2, 1, 4, 0])                # shuffled, repeated, a > b, a == b
    lb = np.array([0, 4, 3, 1, 4, 2, 3, 2, 4])
    win = (37, 1001)
    res = {}
    for mb in (C, 2 * C + 3, E * C):
        p = morse_plan(n, dtype, FREQS, mb)
        try:
            res[mb] = run_all(p, x, None, win, 1)
            assert p.stats()['chunks'] == 3 * -(-E // (mb // C))
            if mb == 2 * C + 3:
                lst = run_all(p, x, (la, lb), win, 1)
        finally:
            p.close()
    for mb in (C, E * C):
        for u, v in zip(res[mb], res[2 * C + 3]):
            assert np.array_equal(u, v), mb
    S, P, phi, lag = res[2 * C + 3]
    assert np.array_equal(lag[..., 0], S.imag)
    lS, lP, lphi, llag = lst
    assert np.array_equal(lP, P)
    for k, (a, b) in enumerate(zip(la, lb)):
        if a == b:                                            # the self pair: its power, exactly; no lag
            assert np.array_equal(lS[:, k].real, P[:, a]) and not np.any(lS[:, k].imag) and not np.any(llag[:, k])
            continue
        q = int(np.flatnonzero((ia == min(a, b)) & (ib == max(a, b)))[0])
        if a < b:
            assert np.array_equal(lS[:, k], S[:, q]) and np.array_equal(lphi[:, k], phi[:, q]), (a, b)
            assert np.array_equal(llag[:, k], lag[:, q]), (a, b)
        else:                                                 # (b, a): the conjugate, the odd lag sums negated
            assert np.array_equal(lS[:, k], np.conj(S[:, q])) and np.array_equal(lphi[:, k], np.conj(phi[:, q])), (a, b)
            assert np.array_equal(llag[:, k] * [-1, 1, 1, -1], lag[:, q]), (a, b)
    # the 17-channel tiling: a short list against all pairs
    C = 17
    x, _ = oracle_rows(n, E, C, dtype, FREQS3)
    ia, ib = all_pairs(C)
    sa, sb = np.array([0, 2, 5, 15, 0]), np.array([16, 2, 11, 16, 1])
    p = morse_plan(n, dtype, FREQS3, 2 * C + 3)
    try:
        full = run_all(p, x, None, win, 1)
        short = run_all(p, x, (sa, sb), win, 1)
    finally:
        p.close()
    assert np.array_equal(short[1], full[1])
    for k, (a, b) in enumerate(zip(sa, sb)):
        if a == b:
            assert np.array_equal(short[0][:, k].real, full[1][:, a])
            continue
        q = int(np.flatnonzero((ia == a) & (ib == b))[0])
        for u, v in zip((short[0], short[2], short[3]), (full[0], full[2], full[3])):
            assert np.array_equal(u[:, k], v[:, q]), (a, b)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_device_tensors_edge_cases_and_errors(dtype):
    """T3: device tensors equal the host call; empty window, E = 0, P = 0; T5: bad arguments raise and
    the plan still works."""
    import torch
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    P, F = len(ia), len(FREQS)
    win = (37, 1001)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        host = run_all(p, x, None, win, 1)
        tx = torch.from_numpy(np.array(x)).cuda()
        tS = torch.full((E, P, F), float('nan'), dtype=torch.complex128, device='cuda')
        tP = torch.full((E, C, F), float('nan'), dtype=torch.float64, device='cuda')
        tphi = torch.full((E, P, F), float('nan'), dtype=torch.complex128, device='cuda')
        tlag = torch.full((E, P, F, 4), float('nan'), dtype=torch.float64, device='cuda')
        out = p.execute_conn_time(tx, None, win, out=(tS, tP), out_kind='cross_sum')
        assert out[0] is tS and out[1] is tP
        assert p.execute_conn_time(tx, None, win, out=tphi, out_kind='plv_sum') is tphi
        assert p.execute_conn_time(tx, None, win, out=tlag, out_kind='lag_sum') is tlag
        for t, h in zip((tS, tP, tphi, tlag), host):
            assert np.array_equal(t.cpu().numpy(), h)
        tS2 = torch.full((E, P, F), float('nan'), dtype=torch.complex128, device='cuda')
        p.execute_conn_time(tx, None, win, out=(tS2, None), out_kind='cross_sum')       # no power sums
        assert np.array_equal(tS2.cpu().numpy(), host[0])
        # window=None is the whole row; step = 3
        full = p.execute_conn_time(x, out_kind='lag_sum')
        assert np.array_equal(full, p.execute_conn_time(x, window=(0, n), out_kind='lag_sum'))
        assert p.execute_conn_time(x, window=(1, 1000), step=3, out_kind='lag_sum').shape == (E, P, F, 4)
        # an empty window: zero sums; no epochs, no pairs: empty outputs
        for kind in KINDS:
            z = p.execute_conn_time(x, window=(n, n), out_kind=kind)
            for a in (z if kind == 'cross_sum' else (z,)):
                assert not np.any(a) and a.shape[0] == E
        S0, P0 = p.execute_conn_time(x[:0], out_kind='cross_sum')
        assert S0.shape == (0, P, F) and P0.shape == (0, C, F)
        assert p.execute_conn_time(x[:0], out_kind='lag_sum').shape == (0, P, F, 4)
        Sn, Pn = p.execute_conn_time(x, ([], []), win, out_kind='cross_sum')
        assert Sn.shape == (E, 0, F) and np.array_equal(Pn, host[1])
        assert p.execute_conn_time(x, ([], []), win, out_kind='plv_sum').shape == (E, 0, F)
        assert p.stats()['reduce_path'] == L.NW_REDUCE_CONN_TIME
        # errors
        for bad in ((-1, 5), (6, 5), (0, n + 1), (0.5, 3), (1,), 7):
            with pytest.raises(ValueError, match='window'):
                p.execute_conn_time(x, window=bad)
        for step in (0, -1, 1.5):
            with pytest.raises(ValueError, match='step'):
                p.execute_conn_time(x, step=step)
        for kind in ('wpli', 'coherence', 'cwt'):
            with pytest.raises(ValueError, match='out_kind'):
                p.execute_conn_time(x, out_kind=kind)
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_conn_time(x, out=np.empty((E, P, F), dtype=np.complex128), out_kind='lag_sum')
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_conn_time(x, out=(np.empty((E, P, F)), np.empty((E, C, F))), out_kind='cross_sum')
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_conn_time(x, out=np.empty((P, F, 4)), out_kind='lag_sum')
        with pytest.raises(ValueError, match='indices'):
            p.execute_conn_time(x, ([0], [C]))
        with pytest.raises(ValueError, match='epochs, channels'):
            p.execute_conn_time(x.reshape(E * C, n))
        with pytest.raises(ValueError, match='output'):
            p.execute_conn_time(tx, out_kind='lag_sum')
        with pytest.raises(ValueError, match='float64'):
            p.execute_conn_time(tx, out=tphi, out_kind='lag_sum')
        with pytest.raises(ValueError, match='hold'):
            p.execute_conn_time(tx, out=tlag[:2], out_kind='lag_sum')
        import ctypes
        V_ = ctypes.c_void_p
        xc = np.ascontiguousarray(x)
        rc = L.lib().nw_execute_conn_time(p.handle, xc.ctypes.data_as(V_), E, C, ia.ctypes.data_as(V_),
                                          ia.ctypes.data_as(V_), len(ia), 0, n, 1, host[3].copy().ctypes.data_as(V_),
                                          host[1].copy().ctypes.data_as(V_), L.NW_OUT_LAG_SUM, L.NW_MEM_HOST)
        assert rc == L.NW_E_INVALID and b'out_power must be NULL' in L.lib().nw_last_error()
        small = morse_plan(n, dtype, FREQS, C - 1)
        try:
            with pytest.raises(ValueError, match='max_batch'):
                small.execute_conn_time(x)
        finally:
            small.close()
        again = run_all(p, x, None, win, 1)                                           # the plan still works
        for u, v in zip(again, host):
            assert np.array_equal(u, v)
        # ... and the epoch-axis call on the same plan is what it was
        assert p.execute_conn(x, out_kind='lag_sum').shape == (P, F, n, 4)
        assert p.stats()['reduce_path'] == L.NW_REDUCE_CONN
    finally:
        p.close()


T4_CASES = [(1024, 'float32', (0, 1024)), (1024, 'float32', (37, 1001)), (1201, 'float32', (0, 1201)),
            (1201, 'float32', (37, 1001)), (1024, 'float64', (0, 1024)), (1024, 'float64', (37, 1001)),
            (1201, 'float64', (0, 1201)), (1201, 'float64', (37, 1001))]


@pytest.mark.parametrize('case', T4_CASES, ids=[f'{n}-{d}-{w[0]}' for n, d, w in T4_CASES])
def test_measures(case):
    """T4."""
    n, dtype, win = case
    E, C = 3, 5
    x, y = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    idx = np.arange(*win)
    T = len(idx)
    A = np.max(np.abs(y), axis=(2, 3))
    AB = (A[:, ia] * A[:, ib])[:, :, None]
    rS, rP, rphi, rlag, m, _, _ = ref_sums(y, ia, ib, idx)
    K = np.sum(np.abs(m) < vis_of(dtype) * AB[..., None], axis=-1)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        S, P, phi, lag = run_all(p, x, None, win, 1)
    finally:
        p.close()
    src = {'cross_sum': (S, rS), 'plv_sum': (phi, rphi), 'lag_sum': (lag, rlag)}
    if dtype == 'float64':
        for kind in MEASURES:
            g, r = src[CONN_OUTS[kind] if kind in CONN_OUTS else LAG_OUTS[kind]]
            dv = np.abs(finalize_conn_time(kind, g, P, ia, ib, T) - finalize_conn_time(kind, r, rP, ia, ib, T)).max()
            print(f'n={n} {win} fp64 {kind}: {dv:.2e}')
            assert dv <= 1e-7, (kind, dv)
        return
    bw = rlag[..., 1] / (T * AB) - 2 * tol
    bc = np.sqrt(rP[:, ia] * rP[:, ib]) / (T * AB) - 2 * tol
    with np.errstate(divide='ignore'):
        bw, bc = np.where(bw > 0, 4 * tol / bw, np.inf), np.where(bc > 0, 4 * tol / bc, np.inf)
    okw, okc = bw <= 0.05, bc <= 0.05
    share_w, share_c = okw.mean(axis=(0, 2)), okc.mean(axis=(0, 2))               # per pair, on the reference alone
    assert np.all(share_w >= 0.7) and np.all(share_c >= 0.85), (share_w.min(), share_c.min())
    dw = np.abs(finalize_conn_time('wpli', lag, None, ia, ib, T) - finalize_conn_time('wpli', rlag, None, ia, ib, T))
    dc = np.abs(finalize_conn_time('coherence', S, P, ia, ib, T) - finalize_conn_time('coherence', rS, rP, ia, ib, T))
    print(f'n={n} {win} fp32: wpli asserted at {share_w.min():.2f}+ of every pair, worst {np.max(dw[okw] / bw[okw]):.3f} '
          f'of its bound; coherence at {share_c.min():.2f}+, worst {np.max(dc[okc] / bc[okc]):.3f} of its bound')
    assert np.all(dw[okw] <= bw[okw]) and np.all(dc[okc] <= bc[okc])
    dpli = np.abs(finalize_conn_time('pli', lag, None, ia, ib, T) - finalize_conn_time('pli', rlag, None, ia, ib, T))
    ddpli = np.abs(finalize_conn_time('dpli', lag, None, ia, ib, T) - finalize_conn_time('dpli', rlag, None, ia, ib, T))
    assert np.all(dpli <= 2 * K / T + 1e-15) and np.all(ddpli <= K / T + 1e-15)


def test_class_layer():
    """T5: connectivity_time_batch is finalize_conn_time of Plan.execute_conn_time, with device decim and with
    host decim; average; EpochsWavelet's padding."""
    E, C = 3, 5
    ia, ib = all_pairs(C)
    # device decim: n = 4096, decim 4, window in full-rate samples
    n, dtype = 4096, 'float32'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype)
    win = (150, 4001)
    t0, t1, step, T = time_window(n, 4, win, True)
    assert (t0, t1, step, T) == (38, 1001, 1, 963)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, decim=4)
    try:
        sums = {k: p.execute_conn_time(x, None, (t0, t1), step, out_kind=k) for k in KINDS}
    finally:
        p.close()
    for out in list(CONN_OUTS) + list(LAG_OUTS):
        need = CONN_OUTS[out] if out in CONN_OUTS else LAG_OUTS[out]
        s, pw = sums[need] if need == 'cross_sum' else (sums[need], None)
        want = finalize_conn_time(out, s, pw, ia, ib, T)
        got = w.connectivity_time_batch(x, FREQS, out=out, window=win, decim=4)
        if out == 'cross_sum':
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            continue
        assert np.array_equal(got, want, equal_nan=True), out
        assert got.shape == ((E, len(ia), len(FREQS), 4) if out == 'lag_sum' else (E, len(ia), len(FREQS))), out
        if not out.endswith('_sum'):
            avg = w.connectivity_time_batch(x, FREQS, out=out, window=win, decim=4, average=True)
            assert avg.shape == (len(ia), len(FREQS)) and np.array_equal(avg, want.mean(axis=0), equal_nan=True), out
    assert len(w._plans) == 1
    st = w.plan_stats()[0]
    assert st['reduce_path'] == L.NW_REDUCE_CONN_TIME and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_decim_kernel'
    coh = w.connectivity_time_batch(x, FREQS, out='coherence', indices=([1, 2], [1, 0]), window=win, decim=4)
    assert np.array_equal(coh[:, 0], np.ones((E, len(FREQS)))) and np.all(coh[:, 1] <= 1 + 1e-12)
    # host decim: the rocFFT engine has no device decimation: a full-rate plan, step = decim
    n, dtype = 1000, 'float64'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype, engine='rocfft')
    win = (37, 990)
    t0, t1, step, T = time_window(n, 4, win, False)
    assert (t0, t1, step, T) == (40, 990, 4, 238)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, engine='rocfft')
    try:
        sums = {k: p.execute_conn_time(x, None, (t0, t1), step, out_kind=k) for k in KINDS}
    finally:
        p.close()
    for out in ('coherence', 'imcoh', 'csd', 'plv', 'wpli', 'dpli', 'wpli2_debiased', 'ciplv', 'ppc', 'lag_sum'):
        need = CONN_OUTS[out] if out in CONN_OUTS else LAG_OUTS[out]
        s, pw = sums[need] if need == 'cross_sum' else (sums[need], None)
        got = w.connectivity_time_batch(x, FREQS, out=out, window=win, decim=4)
        assert np.array_equal(got, finalize_conn_time(out, s, pw, ia, ib, T)), out
    full = w.connectivity_time_batch(x, FREQS, out='wpli')
    assert np.array_equal(full, w.connectivity_time_batch(x, FREQS, out='wpli', window=(0, n)))
    # the finalisers it is made of
    k = 3
    four = np.stack([sums['cross_sum'][0][:, k].real, sums['cross_sum'][0][:, k].imag, sums['cross_sum'][1][:, ia[k]],
                     sums['cross_sum'][1][:, ib[k]]], axis=-1)
    assert np.array_equal(w.connectivity_time_batch(x, FREQS, out='coherence', window=win, decim=4)[:, k],
                          finalize_pair('coherence', four, T))
    assert np.array_equal(w.connectivity_time_batch(x, FREQS, out='wpli', window=win, decim=4)[:, k],
                          finalize_lag('wpli', sums['lag_sum'][:, k], T))
    # EpochsWavelet: padding in seconds, channels picked by name
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)                 # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype, engine='rocfft'))
    sub = np.ascontiguousarray(x[:, :3])
    idx = ([2, 0], [0, 1])
    for method in ('coherence', 'wpli', 'plv', 'ppc'):
        assert np.array_equal(ew.connectivity_time(['a', 'b', 'c'], FREQS, method=method, padding=0.0371),
                              w.connectivity_time_batch(sub, FREQS, out=method, window=(37, n - 37))), method
        assert np.array_equal(ew.connectivity_time(['a', 'b', 'c'], FREQS, method=method, indices=idx, padding=0.1,
                                                   decim=4, average=True),
                              w.connectivity_time_batch(sub, FREQS, out=method, indices=idx, window=(100, 900), decim=4,
                                                        average=True)), method
    assert np.array_equal(ew.connectivity_time(['a', 'b', 'c'], FREQS), w.connectivity_time_batch(sub, FREQS))
    with pytest.raises(ValueError, match='padding'):
        ew.connectivity_time(['a', 'b'], FREQS, padding=0.5)


def test_conn_time_under_bounds_checks():
    """T6: the debug library (kernel bounds checks, nw_dcheck.h) on n = 1024, on a tail tile (n = 1201) and on
    several pair tiles with partial ones (C = 17), every kind, three windows and a short list: no check fails."""
    body = ('rng = np.random.default_rng(1)\n'
            'for tag, n, E, C, dt in (("a", 1024, 3, 5, "float32"), ("b", 1201, 3, 5, "float64"), ("c", 1024, 3, 17, "float64")):\n'
            '    x = rng.standard_normal((E, C, n)).astype(dt)\n'
            '    p = nw.Plan(n, 3, dt, max_batch=2 * C + 3)\n'
            '    p.set_wavelet("morse", [17.5, 3.], np.array([3., 30., 200.]), L.trans_grid(n / 1000., 1000., False))\n'
            '    ok = True\n'
            '    for win, step in ((None, 1), ((37, 1001), 1), ((0, 1), 1), ((5, n), 4), ((9, 9), 1)):\n'
            '        for kind in ("cross_sum", "plv_sum", "lag_sum"):\n'
            '            full = p.execute_conn_time(x, None, win, step, out_kind=kind)\n'
            '            short = p.execute_conn_time(x, ([C - 1, 0, 2], [0, 0, 2]), win, step, out_kind=kind)\n'
            '            for a in (full if kind == "cross_sum" else (full,)) + (short if kind == "cross_sum" else (short,)):\n'
            '                ok = ok and bool(np.all(np.isfinite(a))) and a.shape[0] == E\n'
            '    print("ok", tag, ok)\n'
            '    p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok a True' in lines and 'ok b True' in lines and 'ok c True' in lines, lines
