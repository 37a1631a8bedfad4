"""GPU tests of envelope correlation: nw_execute_env_time (nw_env_time_kernel and nw_env_chan_kernel,
nw_env.hip) through Plan.execute_env_time, engine.finalize_env, WaveletBase.envelope_correlation_batch and
EpochsWavelet.envelope_correlation.

For epoch e, channels c with rows y_e,c (F, n_out), a pair (a, b), a window of T samples s_j = t0 + j step and,
per sample, A_c = |y_c|, the unit phasors w_c = y_c / |y_c|, s = |Im w_a conj(w_b)|, u = A_a s, v = A_b s:
    env_sum       sum_j A_a A_b                                                   (E, P, F)
    env_orth_sum  sum_j of u, u^2, u A_b, v, v^2, v A_a                            (E, P, F, 6)
    chan          sum_j of A_c, re^2 + im^2                                        (E, C, F, 2)
References are formed here from oracle.nw_oracle in complex128.  Inputs (the lagged recipe of epoch_cases.py), cases,
windows, max_batch = 2 C + 3 and tol (1e-12 fp64, 1e-5 fp32, 2e-5 on chirp lengths) are those of
test_gpu_conn_time.py, and the cached oracle rows are shared with it; Amax_c is the signal's max |y| over (F, N) of the undecimated rows.

  T1  against the oracle, first-order bounds.  Per sample, with eta_c = 2 tol Amax_c, theta_c = eta_c / |y_c|,
      sigma = min(1, theta_a + theta_b + theta_a theta_b), du = eta_a s + |y_a| sigma + eta_a sigma (dv likewise):
        |d sum u| <= sum du;  |d sum u^2| <= sum (2 u du + du^2);  |d sum u A_b| <= sum (u eta_b + |y_b| du + du eta_b);
        |d sum A_a A_b| <= sum (|y_a| eta_b + |y_b| eta_a + eta_a eta_b);  |d sum A| <= T eta_c;
        |d sum A^2| <= 2 tol T Amax_c^2 (dP of the sibling file)
      each plus 1e-13 times the sum of the term magnitudes.  On the reference alone, for the listed windows of
      more than one sample: sum sigma <= 0.02 T.
  T2  fp64, the plan's own rows reduced in numpy in the contract's order: chan[..., 1] array_equal; the sums
      that pass through hypot and the divisions within 1e-13 T Ahat_a (sum u), 1e-13 T Ahat_a^2 (sum u^2),
      1e-13 T Ahat_a Ahat_b (sum u A_b, sum A_a A_b), 1e-13 T Ahat (sum A), Ahat the row's max |y| over the window.
  T3  fp64 device identities, bit for bit.
  T4  measures: the T1 bounds propagated through Pearson's formula (pearson_bound below; for sum A^2 the per-sample
      first-order form sum (2 |y| eta + eta^2), which the contract |dy| <= eta / 2 gives); fp32 asserted where the
      bound is <= 0.05, a region that covers >= 0.80 (aec) / 0.75 (aec_orth) of every pair's (e, f) (asserted on
      the reference alone); fp64 every finalised kind within its propagated bound + 1e-9 (T 2^-53 = 1.1e-13 of
      summation rounding, times sum x^2 / var <= 830, times four sums).
  T5  the layers; T6 the debug library."""
import numpy as np
import pytest

from epoch_cases import (FREQS, FREQS3, OVER_TIME, SHAPES, FakeEpochs, forms, lane_sum, morse_plan,
                         run_under_bounds_checks, tol_of, windows_of)
from epoch_cases import lagged_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import ENV_OUTS, all_pairs, finalize_env, time_window  # noqa: E402

KINDS = ('env_sum', 'env_orth_sum')
MEASURES = ('aec', 'aec_directed', 'aec_orth', 'aec_orth_signed')


def run_both(p, x, indices, win, step):
    """(plain (E, P, F), orth (E, P, F, 6), chan (E, C, F, 2)) of one window; the two calls' chan are equal."""
    plain, chan = p.execute_env_time(x, indices, win, step, out_kind='env_sum')
    orth, chan2 = p.execute_env_time(x, indices, win, step, out_kind='env_orth_sum')
    assert np.array_equal(chan, chan2)
    return plain, orth, chan


def ref_env(y, A, ia, ib, idx, tol):
    """The oracle's sums over the samples ``idx`` of rows y (E, C, F, n) and their T1 bounds:
    (plain, orth, chan), (bplain, borth, bchan, bsq), sum sigma (E, P, F)."""
    yw = y[..., idx]
    T = len(idx)
    mag = np.abs(yw)
    eta = 2 * tol * A[:, :, None, None]                             # (E, C, 1, 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = yw / mag
        theta = eta / mag
    Aa, Ab, wa, wb = mag[:, ia], mag[:, ib], w[:, ia], w[:, ib]
    ea, eb, ta, tb = eta[:, ia], eta[:, ib], theta[:, ia], theta[:, ib]
    s = np.abs((wa * np.conj(wb)).imag)
    sigma = np.minimum(1., ta + tb + ta * tb)
    u, v = Aa * s, Ab * s
    du, dv = ea * s + Aa * sigma + ea * sigma, eb * s + Ab * sigma + eb * sigma
    terms = [u, u * u, u * Ab, v, v * v, v * Aa]
    bounds = [du, 2 * u * du + du * du, u * eb + Ab * du + du * eb, dv, 2 * v * dv + dv * dv, v * ea + Aa * dv + dv * ea]
    orth = np.stack([t.sum(-1) for t in terms], axis=-1)
    borth = np.stack([b.sum(-1) + 1e-13 * t.sum(-1) for b, t in zip(bounds, terms)], axis=-1)
    plain = (Aa * Ab).sum(-1)
    bplain = (Aa * eb + Ab * ea + ea * eb).sum(-1) + 1e-13 * plain
    chan = np.stack([mag.sum(-1), (yw.real ** 2 + yw.imag ** 2).sum(-1)], axis=-1)
    e1 = eta[..., 0]                                                # (E, C, 1)
    bchan = np.stack([T * e1 + 1e-13 * chan[..., 0], 2 * tol * T * A[:, :, None] ** 2 + 1e-13 * chan[..., 1]], axis=-1)
    # T4 propagates the per-sample first-order form of the last bound, as for every other sum:
    # |d |y|^2| <= 2 |y| eta + eta^2 (|dy| <= eta / 2); summed it is the tighter one wherever mean |y| < Amax / 2
    bsq = (2 * mag * eta + eta * eta).sum(-1) + 1e-13 * chan[..., 1]
    return (plain, orth, chan), (bplain, borth, bchan, bsq), sigma.sum(-1)


def check_t1(name, got, ref, bounds, ssig, T, listed):
    names = ('plain', 'orth', 'chan')
    if T > 1 and listed:                                            # on the reference alone
        assert np.all(ssig <= 0.02 * T), (name, ssig.max() / T)
    print(f'{name} T={T}: reference: sum sigma <= {ssig.max() / max(T, 1):.4f} T')
    for g, r, b, nm in zip(got, ref, bounds, names):
        assert g.shape == r.shape and g.dtype == np.float64, (name, nm, g.shape, r.shape)
        d = np.abs(g - r)
        with np.errstate(invalid='ignore', divide='ignore'):
            worst = np.nanmax(np.where(b > 0, d / b, 0.), axis=tuple(range(d.ndim - 1)) if nm != 'plain' else None)
        print(f'{name} T1 {nm}: worst share of the bound {np.round(worst, 4)}')
        assert np.all(d <= b), (name, nm, float(np.max(d - b)))


def own_env(rows, ia, ib, idx):
    """(plain, orth, chan) of the plan's own complex128 rows (E, C, F, n_out) in the contract's order, every
    product and every term a separate numpy operation; and Ahat (E, C, F), the rows' max |y| over the window."""
    yw = rows[..., idx]
    re, im = np.ascontiguousarray(yw.real), np.ascontiguousarray(yw.imag)
    with np.errstate(invalid='ignore', divide='ignore'):
        h = np.hypot(re, im)
        ur, ui = re / h, im / h
    Aa, Ab = h[:, ia], h[:, ib]
    t3, t4 = ui[:, ia] * ur[:, ib], ur[:, ia] * ui[:, ib]
    q = np.abs(t3 + (-t4))
    u, v = Aa * q, Ab * q
    orth = np.stack([lane_sum(u), lane_sum(u * u), lane_sum(u * Ab), lane_sum(v), lane_sum(v * v), lane_sum(v * Aa)],
                    axis=-1)
    p1, p2 = re * re, im * im
    chan = np.stack([lane_sum(h), lane_sum(p1 + p2)], axis=-1)
    return lane_sum(Aa * Ab), orth, chan, h.max(axis=-1)


# (id, n, dtype, E, C, freqs, plan keywords, device decim, host decim, kernel of the form): test_gpu_conn_time.py's
CASES = []
for name, n, dtype, kw, decim, host_decim, kernel in forms(*OVER_TIME):
    E, C, freqs = SHAPES.get(name, (3, 5, FREQS))
    CASES.append((name, n, dtype, E, C, freqs, kw, decim, host_decim, kernel))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 for every case and window, T2 for the fp64 cases; every pair a < b; max_batch = 2 C + 3."""
    name, n, dtype, E, C, freqs, kw, decim, host_decim, kernel = case
    x, y = oracle_rows(n, E, C, dtype, freqs)
    A = np.max(np.abs(y), axis=(2, 3))                            # (E, C), of the undecimated rows
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    n_out = n // decim
    F = len(freqs)
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        assert p.n_out == n_out
        got = {}
        for wname, win, step in windows_of(n, n_out, host_decim):
            got[wname] = (win, step, run_both(p, x, None, win, step))
            st = p.stats()
            assert st['reduce_path'] == L.NW_REDUCE_ENV and L.KERNEL_NAMES[st['kernel']] == kernel, (name, st)
        assert st['chunks'] == 2 * len(got) * -(-E // 2), (name, st)
        rows = None
        if dtype == 'float64':
            rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, F, n_out)
    finally:
        p.close()
    for wname, (win, step, sums) in got.items():
        idx = np.arange(win[0], win[1], step)
        T = len(idx)
        assert T == L.conn_time_count(n_out, win[0], win[1], step)
        plain, orth, chan = sums
        assert plain.shape == (E, len(ia), F) and orth.shape == (E, len(ia), F, 6) and chan.shape == (E, C, F, 2)
        if T == 0:                                                # an empty window: zero sums
            assert not np.any(plain) and not np.any(orth) and not np.any(chan), (name, wname)
            continue
        ref, bounds, ssig = ref_env(y, A, ia, ib, idx * decim, tol)
        check_t1(f'{name} {wname}', sums, ref, bounds, ssig, T, wname != 'stride')
        if rows is not None:                                      # T2
            oplain, oorth, ochan, Ah = own_env(rows, ia, ib, idx)
            assert np.array_equal(chan[..., 1], ochan[..., 1]), (name, wname)
            Aa, Ab = Ah[:, ia], Ah[:, ib]
            lim = 1e-13 * T * np.stack([Aa, Aa * Aa, Aa * Ab, Ab, Ab * Ab, Aa * Ab], axis=-1)
            d = np.abs(orth - oorth)
            dp, dc = np.abs(plain - oplain), np.abs(chan[..., 0] - ochan[..., 0])
            print(f'{name} {wname} T2: sum |y|^2 equal bit for bit; of the 1e-13 T limits: orth '
                  f'{np.round((d / lim).max(axis=(0, 1, 2)), 4)} plain {(dp / (1e-13 * T * Aa * Ab)).max():.4f} '
                  f'sum A {(dc / (1e-13 * T * Ah)).max():.4f}')
            assert np.all(d <= lim), (name, wname)
            assert np.all(dp <= 1e-13 * T * Aa * Ab) and np.all(dc <= 1e-13 * T * Ah), (name, wname)


def test_device_identities_bit_for_bit():
    """T3, fp64."""
    n, dtype, E, C = 1024, 'float64', 3, 5
    F = len(FREQS)
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    la = np.array([4, 0, 3, 3, 0, 2, 1, 4, 0])                    # shuffled, repeated, a > b, a == b
    lb = np.array([0, 4, 3, 1, 4, 2, 3, 2, 4])
    res = {}
    for mb in (C, 2 * C + 3, E * C):
        p = morse_plan(n, dtype, FREQS, mb)
        try:
            res[mb] = run_both(p, x, None, (37, 1001), 1)
            assert p.stats()['chunks'] == 2 * -(-E // (mb // C))
            if mb == 2 * C + 3:
                lst = run_both(p, x, (la, lb), (37, 1001), 1)
                for win, step in (((37, 1001), 1), ((0, n), 1), ((5, n - 3), 4), ((0, 1), 1)):
                    chan = p.execute_env_time(x, ([], []), win, step, out_kind='env_sum')[1]
                    # the per-channel sums are nw_execute_pac's amplitude sums and nw_execute_conn_time's power
                    amp = p.execute_pac(x, None, [0], np.arange(F), win, step)[1]
                    power = p.execute_conn_time(x, ([], []), win, step, out_kind='cross_sum')[1]
                    assert np.array_equal(chan[..., 0], amp[..., 0]) and np.array_equal(chan[..., 1], amp[..., 1]), win
                    assert np.array_equal(chan[..., 1], power), win
        finally:
            p.close()
    for mb in (C, E * C):                                         # any chunking
        for u, v in zip(res[mb], res[2 * C + 3]):
            assert np.array_equal(u, v), mb
    plain, orth, chan = res[2 * C + 3]
    lplain, lorth, lchan = lst
    assert np.array_equal(lchan, chan)
    for k, (a, b) in enumerate(zip(la, lb)):                      # any index list
        if a == b:                                                # a self pair: six zeros (+0.0)
            assert not np.any(lorth[:, k]) and not np.any(np.signbit(lorth[:, k])), (a, b)
            continue
        q = int(np.flatnonzero((ia == min(a, b)) & (ib == max(a, b)))[0])
        assert np.array_equal(lplain[:, k], plain[:, q]), (a, b)  # the plain sum does not see the order
        if a < b:
            assert np.array_equal(lorth[:, k], orth[:, q]), (a, b)
        else:                                                     # (b, a): the u triple and the v triple change places
            assert np.array_equal(lorth[:, k][..., [3, 4, 5, 0, 1, 2]], orth[:, q]), (a, b)
    # the 17-channel tiling: a short list against all pairs
    C = 17
    x, _ = oracle_rows(n, E, C, dtype, FREQS3)
    ia, ib = all_pairs(C)
    sa, sb = np.array([0, 2, 5, 15, 0]), np.array([16, 2, 11, 16, 1])
    assert L.conn_tiles(C, ia, ib)[1] == 3
    p = morse_plan(n, dtype, FREQS3, 2 * C + 3)
    try:
        full = run_both(p, x, None, (37, 1001), 1)
        short = run_both(p, x, (sa, sb), (37, 1001), 1)
    finally:
        p.close()
    assert np.array_equal(short[2], full[2])
    for k, (a, b) in enumerate(zip(sa, sb)):
        if a == b:
            assert not np.any(short[1][:, k])
            continue
        q = int(np.flatnonzero((ia == a) & (ib == b))[0])
        assert np.array_equal(short[0][:, k], full[0][:, q]) and np.array_equal(short[1][:, k], full[1][:, q]), (a, b)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_device_tensors_edge_cases_and_errors(dtype):
    """T3: device tensors equal the host call; empty window, E = 0, P = 0; T5: bad arguments raise, the plan
    still works and execute_conn_time on the same plan returns what it did before."""
    import torch
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    P, F = len(ia), len(FREQS)
    win = (37, 1001)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        lag_before = p.execute_conn_time(x, None, win, out_kind='lag_sum')
        host = run_both(p, x, None, win, 1)
        tx = torch.from_numpy(np.array(x)).cuda()
        tplain = torch.full((E, P, F), float('nan'), dtype=torch.float64, device='cuda')
        torth = torch.full((E, P, F, 6), float('nan'), dtype=torch.float64, device='cuda')
        tchan = torch.full((E, C, F, 2), float('nan'), dtype=torch.float64, device='cuda')
        out = p.execute_env_time(tx, None, win, out=(tplain, tchan), out_kind='env_sum')
        assert out[0] is tplain and out[1] is tchan
        assert np.array_equal(tplain.cpu().numpy(), host[0]) and np.array_equal(tchan.cpu().numpy(), host[2])
        tchan.fill_(float('nan'))
        p.execute_env_time(tx, None, win, out=(torth, tchan))
        assert np.array_equal(torth.cpu().numpy(), host[1]) and np.array_equal(tchan.cpu().numpy(), host[2])
        torth.fill_(float('nan'))
        p.execute_env_time(tx, None, win, out=(torth, None))                              # no per-channel sums
        assert np.array_equal(torth.cpu().numpy(), host[1])
        # window=None is the whole row; step = 3; the default kind is the orthogonalised one
        full = p.execute_env_time(x)
        assert full[0].shape == (E, P, F, 6)
        assert np.array_equal(full[0], p.execute_env_time(x, window=(0, n), out_kind='env_orth_sum')[0])
        assert p.execute_env_time(x, window=(1, 1000), step=3)[0].shape == (E, P, F, 6)
        # an empty window: zero sums; no epochs, no pairs: empty outputs
        for kind in KINDS:
            tail = (6,) if kind == 'env_orth_sum' else ()
            z = p.execute_env_time(x, window=(n, n), out_kind=kind)
            assert not np.any(z[0]) and not np.any(z[1]) and z[0].shape == (E, P, F) + tail
            z = p.execute_env_time(x[:0], out_kind=kind)
            assert z[0].shape == (0, P, F) + tail and z[1].shape == (0, C, F, 2)
            z = p.execute_env_time(x, ([], []), win, out_kind=kind)
            assert z[0].shape == (E, 0, F) + tail and np.array_equal(z[1], host[2])
        assert p.stats()['reduce_path'] == L.NW_REDUCE_ENV
        # errors
        for bad in ((-1, 5), (6, 5), (0, n + 1), (0.5, 3), (1,), 7):
            with pytest.raises(ValueError, match='window'):
                p.execute_env_time(x, window=bad)
        for step in (0, -1, 1.5):
            with pytest.raises(ValueError, match='step'):
                p.execute_env_time(x, step=step)
        for kind in ('aec', 'aec_orth', 'lag_sum', 'cwt'):
            with pytest.raises(ValueError, match='out_kind'):
                p.execute_env_time(x, out_kind=kind)
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_env_time(x, out=(np.empty((E, P, F)), None))                        # the plain size for orth
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_env_time(x, out=(np.empty((E, P, F), dtype=np.float32), None), out_kind='env_sum')
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_env_time(x, out=(None, np.empty((E, C, F))), out_kind='env_sum')
        with pytest.raises(ValueError, match='indices'):
            p.execute_env_time(x, ([0], [C]))
        with pytest.raises(ValueError, match='epochs, channels'):
            p.execute_env_time(x.reshape(E * C, n))
        with pytest.raises(ValueError, match='output'):
            p.execute_env_time(tx)
        with pytest.raises(ValueError, match='float64'):
            p.execute_env_time(tx, out=(torth.to(torch.float32), None))
        with pytest.raises(ValueError, match='hold'):
            p.execute_env_time(tx, out=(torth[:2], None))
        import ctypes
        V_ = ctypes.c_void_p
        xc = np.ascontiguousarray(x)
        rc = L.lib().nw_execute_env_time(p.handle, xc.ctypes.data_as(V_), E, C, ia.ctypes.data_as(V_),
                                         ib.ctypes.data_as(V_), len(ia), 0, n, 1, host[1].copy().ctypes.data_as(V_),
                                         None, 2, L.NW_MEM_HOST)
        assert rc == L.NW_E_INVALID and b'env_kind' in L.lib().nw_last_error()
        small = morse_plan(n, dtype, FREQS, C - 1)
        try:
            with pytest.raises(ValueError, match='max_batch'):
                small.execute_env_time(x)
        finally:
            small.close()
        again = run_both(p, x, None, win, 1)                                              # the plan still works
        for u, v in zip(again, host):
            assert np.array_equal(u, v)
        # ... and the phase-lag call on the same plan is what it was
        assert np.array_equal(p.execute_conn_time(x, None, win, out_kind='lag_sum'), lag_before)
        assert p.stats()['reduce_path'] == L.NW_REDUCE_CONN_TIME
    finally:
        p.close()


def pearson_bound(sxy, sx, sy, sxx, syy, dxy, dx, dy, dxx, dyy, T):
    """(r, B): Pearson's r of the reference sums and the first-order bound on its change when every sum moves by
    at most its d..: dcov = dxy + (|sx| dy + |sy| dx + dx dy) / T, dvar = dxx + (2 |sx| dx + dx^2) / T,
    B = dcov / D_lo + |r| (D / D_lo - 1) with D = sqrt(var_x var_y) and D_lo from var - dvar; inf where a
    var - dvar <= 0."""
    cov = sxy - sx * sy / T
    vx, vy = sxx - sx * sx / T, syy - sy * sy / T
    dcov = dxy + (np.abs(sx) * dy + np.abs(sy) * dx + dx * dy) / T
    lx, ly = vx - (dxx + (2 * np.abs(sx) * dx + dx * dx) / T), vy - (dyy + (2 * np.abs(sy) * dy + dy * dy) / T)
    ok = (lx > 0) & (ly > 0)
    D, Dlo = np.sqrt(np.where(ok, vx * vy, 1.)), np.sqrt(np.where(ok, lx * ly, 1.))
    r = np.where(ok, cov / D, 0.)
    return r, np.where(ok, dcov / Dlo + np.abs(r) * (D / Dlo - 1), np.inf)


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
    (rplain, rorth, rchan), (bplain, borth, bchan, bsq), _ = ref_env(y, A, ia, ib, idx, tol)
    bchan = np.stack([bchan[..., 0], bsq], axis=-1)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        plain, orth, chan = run_both(p, x, None, win, 1)
    finally:
        p.close()
    ca, cb, dca, dcb = rchan[:, ia], rchan[:, ib], bchan[:, ia], bchan[:, ib]
    _, B = pearson_bound(rplain, ca[..., 0], cb[..., 0], ca[..., 1], cb[..., 1],
                         bplain, dca[..., 0], dcb[..., 0], dca[..., 1], dcb[..., 1], T)
    _, Bab = pearson_bound(rorth[..., 2], rorth[..., 0], cb[..., 0], rorth[..., 1], cb[..., 1],
                           borth[..., 2], borth[..., 0], dcb[..., 0], borth[..., 1], dcb[..., 1], T)
    _, Bba = pearson_bound(rorth[..., 5], rorth[..., 3], ca[..., 0], rorth[..., 4], ca[..., 1],
                           borth[..., 5], borth[..., 3], dca[..., 0], borth[..., 4], dca[..., 1], T)
    bound = {'aec': B, 'aec_directed': np.stack([Bab, Bba], axis=-1), 'aec_orth': (Bab + Bba) / 2,
             'aec_orth_signed': (Bab + Bba) / 2}
    diff = {}
    for kind in MEASURES:
        src, rsrc = (plain, rplain) if kind == 'aec' else (orth, rorth)
        g, r = finalize_env(kind, src, chan, ia, ib, T), finalize_env(kind, rsrc, rchan, ia, ib, T)
        assert g.shape == r.shape == bound[kind].shape and np.all(np.isfinite(g)) and np.abs(g).max() <= 1 + 1e-6
        diff[kind] = np.abs(g - r)
    if dtype == 'float64':
        for kind in MEASURES:
            over = np.max(diff[kind] - bound[kind])
            print(f'n={n} {win} fp64 {kind}: max diff {diff[kind].max():.2e}, over its bound {over:.2e}')
            assert np.all(diff[kind] <= bound[kind] + 1e-9), (kind, over)
        return
    ok_a, ok_o = bound['aec'] <= 0.05, bound['aec_orth'] <= 0.05
    share_a, share_o = ok_a.mean(axis=(0, 2)), ok_o.mean(axis=(0, 2))             # per pair, on the reference alone
    assert np.all(share_a >= 0.80) and np.all(share_o >= 0.75), (share_a.min(), share_o.min())
    print(f'n={n} {win} fp32: aec asserted at {share_a.min():.3f}+ of every pair, worst '
          f'{np.max(diff["aec"][ok_a] / bound["aec"][ok_a]):.3f} of its bound; aec_orth at {share_o.min():.3f}+, worst '
          f'{np.max(diff["aec_orth"][ok_o] / bound["aec_orth"][ok_o]):.3f} of its bound')
    assert np.all(diff['aec'][ok_a] <= bound['aec'][ok_a])
    assert np.all(diff['aec_orth'][ok_o] <= bound['aec_orth'][ok_o])


def test_class_layer():
    """T5: envelope_correlation_batch is finalize_env of Plan.execute_env_time, with device decim and with host
    decim; average; EpochsWavelet's padding, names and indices."""
    E, C = 3, 5
    ia, ib = all_pairs(C)
    F = len(FREQS)
    # device decim: n = 4096, decim 4, window in full-rate samples
    n, dtype = 4096, 'float32'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype)
    win = (150, 4001)
    t0, t1, step, T = time_window(n, 4, win, True)
    assert (t0, t1, step, T) == (38, 1001, 1, 963)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, decim=4)
    try:
        sums = {k: p.execute_env_time(x, None, (t0, t1), step, out_kind=k) for k in KINDS}
    finally:
        p.close()
    for out in ENV_OUTS:
        want = finalize_env(out, *sums[ENV_OUTS[out]], ia, ib, T)
        got = w.envelope_correlation_batch(x, FREQS, out=out, window=win, decim=4)
        if out.endswith('_sum'):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), out
            continue
        assert np.array_equal(got, want), out
        assert got.shape == (E, len(ia), F) + ((2,) if out == 'aec_directed' else ()), out
        avg = w.envelope_correlation_batch(x, FREQS, out=out, window=win, decim=4, average=True)
        assert avg.shape == got.shape[1:] and np.array_equal(avg, want.mean(axis=0)), out
    assert len(w._plans) == 1
    st = w.plan_stats()[0]
    assert st['reduce_path'] == L.NW_REDUCE_ENV and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_decim_kernel'
    own = w.envelope_correlation_batch(x, FREQS, indices=([1, 2], [1, 0]), window=win, decim=4)
    assert not np.any(own[:, 0]) and np.all(own[:, 1] > 0) and np.all(own <= 1 + 1e-6)   # the default: aec_orth
    assert np.array_equal(own, w.envelope_correlation_batch(x, FREQS, out='aec_orth', indices=([1, 2], [1, 0]),
                                                            window=win, decim=4))
    # host decim: the rocFFT engine has no device decimation: a full-rate plan, step = decim
    n, dtype = 1000, 'float64'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype, engine='rocfft')
    win = (37, 990)
    t0, t1, step, T = time_window(n, 4, win, False)
    assert (t0, t1, step, T) == (40, 990, 4, 238)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, engine='rocfft')
    try:
        sums = {k: p.execute_env_time(x, None, (t0, t1), step, out_kind=k) for k in KINDS}
    finally:
        p.close()
    for out in MEASURES:
        got = w.envelope_correlation_batch(x, FREQS, out=out, window=win, decim=4)
        assert np.array_equal(got, finalize_env(out, *sums[ENV_OUTS[out]], ia, ib, T)), out
    full = w.envelope_correlation_batch(x, FREQS, out='aec')
    assert np.array_equal(full, w.envelope_correlation_batch(x, FREQS, out='aec', window=(0, n)))
    # EpochsWavelet: padding in seconds, channels picked by name
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)                 # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype, engine='rocfft'))
    sub = np.ascontiguousarray(x[:, :3])
    idx = ([2, 0], [0, 1])
    for method in MEASURES:
        assert np.array_equal(ew.envelope_correlation(['a', 'b', 'c'], FREQS, method=method, padding=0.0371),
                              w.envelope_correlation_batch(sub, FREQS, out=method, window=(37, n - 37))), method
        assert np.array_equal(ew.envelope_correlation(['a', 'b', 'c'], FREQS, method=method, indices=idx, padding=0.1,
                                                      decim=4, average=True),
                              w.envelope_correlation_batch(sub, FREQS, out=method, indices=idx, window=(100, 900),
                                                           decim=4, average=True)), method
    assert np.array_equal(ew.envelope_correlation(['a', 'b', 'c'], FREQS), w.envelope_correlation_batch(sub, FREQS))
    with pytest.raises(ValueError, match='padding'):
        ew.envelope_correlation(['a', 'b'], FREQS, padding=0.5)


def test_env_time_under_bounds_checks():
    """T6: the debug library (kernel bounds checks, nw_dcheck.h) on n = 1024, on a tail tile (n = 1201) and on
    several pair tiles with partial ones (C = 17), both modes, five windows and a short list: no check fails."""
    body = ('rng = np.random.default_rng(1)\n'
            'for tag, n, E, C, dt in (("a", 1024, 3, 5, "float32"), ("b", 1201, 3, 5, "float64"), ("c", 1024, 3, 17, "float64")):\n'
            '    x = rng.standard_normal((E, C, n)).astype(dt)\n'
            '    p = nw.Plan(n, 3, dt, max_batch=2 * C + 3)\n'
            '    p.set_wavelet("morse", [17.5, 3.], np.array([3., 30., 200.]), L.trans_grid(n / 1000., 1000., False))\n'
            '    ok = True\n'
            '    for win, step in ((None, 1), ((37, 1001), 1), ((0, 1), 1), ((5, n), 4), ((9, 9), 1)):\n'
            '        for kind in ("env_sum", "env_orth_sum"):\n'
            '            full = p.execute_env_time(x, None, win, step, out_kind=kind)\n'
            '            short = p.execute_env_time(x, ([C - 1, 0, 2], [0, 0, 2]), win, step, out_kind=kind)\n'
            '            for a in full + short:\n'
            '                ok = ok and bool(np.all(np.isfinite(a))) and a.shape[0] == E\n'
            '    print("ok", tag, ok)\n'
            '    p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok a True' in lines and 'ok b True' in lines and 'ok c True' in lines, lines
