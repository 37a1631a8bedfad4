"""GPU tests of multi-channel connectivity: nw_execute_conn (nw_conn_accumulate_kernel and
nw_conn_power_kernel over each chunk's complex rows, nw_conn.hip) through Plan.execute_conn,
WaveletBase.connectivity_batch and EpochsWavelet.connectivity.

For epochs e, channels c with rows y_e,c (F, n_out) and pairs p = (a, b):
    S_p = sum_e y_a conj(y_b),  P_cc = sum_e |y_c|^2,  Phi_p = sum_e (y_a/|y_a|) conj(y_b/|y_b|)
every sum in fp64 in epoch order.  References are formed here from oracle.nw_oracle in complex128.

Inputs: the plain recipe of epoch_cases.py: rng = default_rng(2300 + n), common = rng.standard_normal((E, 1, n)),
x = 0.6 common + 0.8 rng.standard_normal((E, C, n)); Morse(1000) with its default b, r and the nine
scales FREQS (three, FREQS3, for the C = 17 tile case and the 2^15 case).

Bounds (those of test_gpu_pair.py).  A_e,c: that signal's max|y| over (F, N); tol: 1e-12 fp64,
1e-5 fp32, 2e-5 fp32 on chirp-z lengths.
  T1  |dS_ab| <= 2 tol sum_e A_e,a A_e,b,  |dP_cc| <= 2 tol sum_e A_e,c^2  (pointwise, against the oracle)
  T2  against the same plan's own rows reduced in numpy complex128: 1e-13 sum_e |y_a||y_b| for S
      (1e-13 P_cc for P), 1e-13 E for Phi where every |y| > 0
  T3  v = 0.01: |dplv| <= 2 tol / v where every epoch has |y_a| >= v A and |y_b| >= v A (at least 0.8
      of the points of EVERY pair, asserted on the reference); fp64 |dcoherence| <= 4 tol / v^2 where
      P >= v^2 sum A^2 (every point, asserted on the reference)
The transform rows of the fp32 one-pass kernel at n <= 4096 carry two signals per lane value, so a
signal's fp32 rows depend (in rounding) on its neighbour in the chunk: the exact comparisons between
differently chunked calls are made in fp64, where a row depends on its signal alone."""
import ctypes

import numpy as np
import pytest

from epoch_cases import (EPOCH_AXIS, FREQS, SHAPES, FakeEpochs, forms, morse_plan, run_under_bounds_checks, tol_of)
from epoch_cases import plain_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import PAIR_OUTS, all_pairs, finalize_conn, finalize_pair  # noqa: E402

V = 0.01
DTYPES = ['float32', 'float64']
OUTS = ['cross_sum', 'plv_sum', 'csd', 'coherency', 'coherence', 'imcoh', 'plv']


def sums_of(y, ia, ib):
    """(S (P, F, n), P_cc (C, F, n), Phi (P, F, n)) of complex128 rows (E, C, F, n), added in epoch order."""
    s = np.zeros((len(ia),) + y.shape[2:], dtype=np.complex128)
    phi = np.zeros_like(s)
    power = np.zeros(y.shape[1:])
    with np.errstate(invalid='ignore', divide='ignore'):
        for e in range(y.shape[0]):
            s += y[e][ia] * np.conj(y[e][ib])
            power += np.abs(y[e]) ** 2
            u = y[e] / np.abs(y[e])
            phi += u[ia] * np.conj(u[ib])
    return s, power, phi


def run_conn(n, dtype, freqs, max_batch, x, indices=None, **kw):
    """(cross, power, phi, stats after cross_sum, stats after plv_sum) of one plan."""
    p = morse_plan(n, dtype, freqs, max_batch, **kw)
    try:
        cross, power = p.execute_conn(x, indices, out_kind='cross_sum')
        st_c = p.stats()
        phi = p.execute_conn(x, indices, out_kind='plv_sum')
        st_p = p.stats()
    finally:
        p.close()
    return cross, power, phi, st_c, st_p


# (id, n, dtype, E, C, freqs, plan keywords, decim, kernel of the form): five epochs but for the rows of SHAPES
CASES = []
for name, n, dtype, kw, decim, _, kernel in forms(*EPOCH_AXIS):
    E, C, freqs = SHAPES.get(name, (5, 5, FREQS))
    CASES.append((name, n, dtype, E, C, freqs, kw, decim, kernel))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_conn_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 and T2 for every pair a < b; max_batch = 2 C + 3: chunks of 2, 2, 1 (C = 17: 2, 1) epochs
    and a batch that is no multiple of C."""
    name, n, dtype, E, C, freqs, kw, decim, kernel = case
    x, y = oracle_rows(n, E, C, dtype, freqs)
    y = y[..., ::decim]
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        cross, power = p.execute_conn(x, out_kind='cross_sum')
        st_c = p.stats()
        phi = p.execute_conn(x, out_kind='plv_sum')
        st_p = p.stats()
        rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape((E, C) + y.shape[2:])
    finally:
        p.close()
    P, F, no = len(ia), len(freqs), n // decim
    assert cross.shape == (P, F, no) and cross.dtype == np.complex128
    assert power.shape == (C, F, no) and power.dtype == np.float64
    assert phi.shape == (P, F, no) and phi.dtype == np.complex128
    for st in (st_c, st_p):
        assert st['reduce_path'] == L.NW_REDUCE_CONN, (name, st)
        assert L.KERNEL_NAMES[st['kernel']] == kernel, (name, st)
    assert st_c['chunks'] == -(-E // 2) and st_p['chunks'] == 2 * -(-E // 2), (st_c, st_p)
    if C > 16:
        assert L.conn_tiles(C, ia, ib)[1] == 3
    # T1
    want_s, want_p, _ = sums_of(y, ia, ib)
    A = np.max(np.abs(y), axis=(2, 3))                       # (E, C)
    s_scale = np.sum(A[:, ia] * A[:, ib], axis=0)[:, None, None]
    p_scale = np.sum(A * A, axis=0)[:, None, None]
    es = np.max(np.abs(cross - want_s) / s_scale)
    ep = np.max(np.abs(power - want_p) / p_scale)
    print(f'{name} T1: dS {es / (2 * tol):.3f} dP {ep / (2 * tol):.3f} of the bound (tol {tol:.0e})')
    assert es <= 2 * tol and ep <= 2 * tol, (name, es, ep)
    # T2
    own_s, own_p, own_phi = sums_of(rows, ia, ib)
    mag = np.abs(rows)
    sab = np.zeros((P, F, no))
    for e in range(E):
        sab += mag[e][ia] * mag[e][ib]
    ds, dp = np.abs(cross - own_s), np.abs(power - own_p)
    pos = np.all(mag > 0, axis=0)                            # (C, F, n)
    pos = pos[ia] & pos[ib]
    dphi = np.abs(phi - own_phi)[pos]
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = [np.nanmax(np.where(sab > 0, ds / sab, 0)), np.nanmax(np.where(own_p > 0, dp / own_p, 0)),
                 np.max(dphi) / E]
    print(f'{name} T2: dS {worst[0]:.2e} dP {worst[1]:.2e} dPhi/E {worst[2]:.2e} (bound 1e-13); '
          f'{pos.mean():.3f} of the points have every |y| > 0')
    assert np.all(ds <= 1e-13 * sab) and np.all(dp <= 1e-13 * own_p), (name, worst)
    assert pos.mean() >= 0.5 and np.all(dphi <= 1e-13 * E), (name, worst)


# (the C = 17 shape with the nine scales here: its worst pair then keeps 0.88 of the points, the
# figure the mask bound was set from; with the three scales of the tile case the 3 Hz row alone
# leaves the worst pair 0.71)
T3_CASES = [(1024, 5, 5, FREQS), (1201, 5, 5, FREQS), (1024, 3, 17, FREQS)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', T3_CASES, ids=[f'{n}-{E}x{C}' for n, E, C, _ in T3_CASES])
def test_plv_and_coherence_on_visible_points(shape, dtype):
    """T3 for every pair."""
    n, E, C, freqs = shape
    x, y = oracle_rows(n, E, C, dtype, freqs)
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    A = np.max(np.abs(y), axis=(2, 3))[:, :, None, None]
    seen = np.all(np.abs(y) >= V * A, axis=0)                # (C, F, n): every epoch visible
    vis = seen[ia] & seen[ib]
    per_pair = vis.mean(axis=(1, 2))
    assert np.all(per_pair >= 0.8), per_pair.min()           # on the reference alone
    want_s, want_p, want_phi = sums_of(y, ia, ib)
    cross, power, phi, _, _ = run_conn(n, dtype, freqs, 2 * C + 3, x)
    dplv = np.abs(finalize_conn('plv', phi, None, ia, ib, E) - finalize_conn('plv', want_phi, None, ia, ib, E))
    worst = np.max(dplv[vis])
    print(f'n={n} E={E} C={C} {dtype} T3: visible {per_pair.min():.2f}-{per_pair.max():.2f} per pair; '
          f'dplv {worst:.3e} = {worst / (2 * tol / V):.4f} of the bound')
    assert worst <= 2 * tol / V
    if dtype == 'float64':
        pv = want_p >= V * V * np.sum(A * A, axis=0)
        assert np.all(pv)                                    # on the reference alone
        dcoh = np.abs(finalize_conn('coherence', cross, power, ia, ib, E) -
                      finalize_conn('coherence', want_s, want_p, ia, ib, E))
        print(f'n={n} E={E} C={C} {dtype} T3: dcoherence {np.max(dcoh):.3e} = {np.max(dcoh) / (4 * tol / V ** 2):.2e} '
              'of the bound')
        assert np.max(dcoh) <= 4 * tol / V ** 2


@pytest.mark.parametrize('dtype', DTYPES)
def test_indexed_list_with_reversed_repeated_and_self_pairs(dtype):
    n, E, C = 1024, 5, 6
    x, y = oracle_rows(n, E, C, dtype, FREQS)
    ia = np.array([5, 0, 3, 3, 0, 2])
    ib = np.array([0, 5, 3, 1, 5, 2])
    tol = tol_of(n, dtype)
    cross, power, phi, st, _ = run_conn(n, dtype, FREQS, 2 * C + 3, x, (ia, ib))
    assert st['reduce_path'] == L.NW_REDUCE_CONN
    assert cross.shape == (6, len(FREQS), n) and power.shape == (C, len(FREQS), n)
    # results land in the caller's order: T1 against the oracle for this list
    want_s, want_p, _ = sums_of(y, ia, ib)
    A = np.max(np.abs(y), axis=(2, 3))
    assert np.max(np.abs(cross - want_s) / np.sum(A[:, ia] * A[:, ib], axis=0)[:, None, None]) <= 2 * tol
    assert np.max(np.abs(power - want_p) / np.sum(A * A, axis=0)[:, None, None]) <= 2 * tol
    # (5, 0) and (0, 5): conjugates, exactly; (0, 5) twice: equal, exactly
    assert np.array_equal(cross[0], np.conj(cross[1])) and np.array_equal(phi[0], np.conj(phi[1]))
    assert np.array_equal(cross[1], cross[4]) and np.array_equal(phi[1], phi[4])
    # the self pairs (3, 3) and (2, 2): S real and equal to P_cc, coherence 1, exactly
    for p, c in ((2, 3), (5, 2)):
        assert not np.any(cross[p].imag) and np.array_equal(cross[p].real, power[c])
    coh = finalize_conn('coherence', cross, power, ia, ib, E)
    imc = finalize_conn('imcoh', cross, power, ia, ib, E)
    for p in (2, 5):
        assert np.array_equal(coh[p], np.ones_like(coh[p])) and not np.any(imc[p])


@pytest.mark.parametrize('n', [1024, 1201])
def test_pair_sums_are_the_pair_paths_bit_for_bit(n):
    """fp64 (nw_pair_partials_supported is 0): the sums of a pair are those of nw_execute_pair on
    its per-signal-rows path for the same two channels -- the same terms in the same order."""
    dtype, E, C = 'float64', 5, 5
    assert not L.pair_partials_supported(n, L.NW_F64, L.NW_MORSE, L.NW_OUT_CROSS_SUM)
    assert not L.pair_partials_supported(n, L.NW_F64, L.NW_MORSE, L.NW_OUT_PLV_SUM)
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    cross, power, phi, _, _ = run_conn(n, dtype, FREQS, 2 * C + 3, x)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        for a, b in ((0, 3), (2, 4)):
            k = int(np.flatnonzero((ia == a) & (ib == b))[0])
            sums = p.execute_pair(x[:, a], x[:, b], out_kind='cross_sum')
            assert p.stats()['reduce_path'] == L.NW_REDUCE_ROWS
            plv = p.execute_pair(x[:, a], x[:, b], out_kind='plv_sum')
            assert np.array_equal(cross[k].real, sums[..., 0]) and np.array_equal(cross[k].imag, sums[..., 1]), (a, b)
            assert np.array_equal(power[a], sums[..., 2]) and np.array_equal(power[b], sums[..., 3]), (a, b)
            assert np.array_equal(phi[k], plv), (a, b)
    finally:
        p.close()


@pytest.mark.parametrize('n', [1024, 1201])
def test_chunking_changes_nothing(n):
    """One epoch per chunk (max_batch = C) and all epochs in one chunk (max_batch = E C): the same
    bits (fp64: a row depends on its signal alone)."""
    dtype, E, C = 'float64', 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    one = run_conn(n, dtype, FREQS, C, x)
    all_ = run_conn(n, dtype, FREQS, E * C, x)
    assert one[3]['chunks'] == E and all_[3]['chunks'] == 1
    for got, want in zip(one[:3], all_[:3]):
        assert np.array_equal(got, want)


def test_class_layer():
    """connectivity_batch against cross_batch pair by pair (T2's bounds on the sums; every finalised
    output is finalize_pair of the call's own sums, exactly), decim, EpochsWavelet.connectivity."""
    dtype, n, E, C = 'float64', 1024, 5, 5
    x, y = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    w = nw.Morse(1000, dtype=dtype)
    got = {out: w.connectivity_batch(x, FREQS, out=out) for out in OUTS}
    assert len(w._plans) == 1 and w.plan_stats()[0]['reduce_path'] == L.NW_REDUCE_CONN
    cross, power = got['cross_sum']
    phi = got['plv_sum']
    mag = np.abs(y)
    wp = nw.Morse(1000, dtype=dtype)
    for k, (a, b) in enumerate(zip(ia, ib)):
        sums = wp.cross_batch(x[:, a], x[:, b], FREQS, out='cross_sum')
        plv_sum = wp.cross_batch(x[:, a], x[:, b], FREQS, out='plv_sum')
        sab = np.sum(mag[:, a] * mag[:, b], axis=0)
        assert np.all(np.abs(cross[k] - (sums[..., 0] + 1j * sums[..., 1])) <= 1e-13 * sab), (a, b)
        assert np.all(np.abs(power[a] - sums[..., 2]) <= 1e-13 * sums[..., 2]), (a, b)
        assert np.all(np.abs(power[b] - sums[..., 3]) <= 1e-13 * sums[..., 3]), (a, b)
        assert np.all(np.abs(phi[k] - plv_sum) <= 1e-13 * E), (a, b)
        own = np.stack([cross[k].real, cross[k].imag, power[a], power[b]], axis=-1)
        for out in OUTS[2:]:
            src = phi[k] if PAIR_OUTS[out] == 'plv_sum' else own
            assert np.array_equal(got[out][k], finalize_pair(out, src, E)), (out, a, b)
    for out in OUTS[2:]:
        assert got[out].shape == (len(ia), len(FREQS), n), out
        assert got[out].dtype == (np.complex128 if out in ('csd', 'coherency') else np.float64), out
    assert np.all(got['coherence'] <= 1 + 1e-12)
    # an index list, and EpochsWavelet: positions in ch_names, channels picked from the epochs
    idx = ([2, 0], [0, 1])
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)          # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype))
    sub = np.ascontiguousarray(x[:, :3])
    for method in ('coherence', 'imcoh', 'plv', 'csd'):
        assert np.array_equal(ew.connectivity(['a', 'b', 'c'], FREQS, method=method),
                              w.connectivity_batch(sub, FREQS, out=method)), method
        assert np.array_equal(ew.connectivity(['a', 'b', 'c'], FREQS, method=method, indices=idx),
                              w.connectivity_batch(sub, FREQS, out=method, indices=idx)), method
    # decim: n = 1201 has no device decimation: the undecimated result [..., ::5], exactly
    x5, _ = oracle_rows(1201, E, C, dtype, FREQS)
    w5 = nw.Morse(1000, dtype=dtype)
    for out in ('coherence', 'plv', 'csd', 'plv_sum'):
        full = w5.connectivity_batch(x5, FREQS, out=out)
        dec = w5.connectivity_batch(x5, FREQS, out=out, decim=5)
        assert dec.shape == (len(ia), len(FREQS), 241) and np.array_equal(dec, full[..., ::5]), out
    fs, fp = w5.connectivity_batch(x5, FREQS, out='cross_sum')
    ds, dp = w5.connectivity_batch(x5, FREQS, out='cross_sum', decim=5)
    assert np.array_equal(ds, fs[..., ::5]) and np.array_equal(dp, fp[..., ::5])
    assert len(w5._plans) == 1
    # ... and on the device where supported (n = 4096, decim 4)
    x4, y4 = oracle_rows(4096, E, C, 'float32', FREQS)
    w4 = nw.Morse(1000, dtype='float32')
    s4, p4 = w4.connectivity_batch(x4, FREQS, out='cross_sum', decim=4)
    assert s4.shape == (len(ia), len(FREQS), 1024) and p4.shape == (C, len(FREQS), 1024)
    assert L.KERNEL_NAMES[w4.plan_stats()[0]['kernel']] == 'nw_fused_decim_kernel'
    want_s, want_p, _ = sums_of(y4[..., ::4], ia, ib)
    A = np.max(np.abs(y4), axis=(2, 3))
    assert np.max(np.abs(s4 - want_s) / np.sum(A[:, ia] * A[:, ib], axis=0)[:, None, None]) <= 2e-5
    assert np.max(np.abs(p4 - want_p) / np.sum(A * A, axis=0)[:, None, None]) <= 2e-5


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_tensors_equal_the_host_call_bit_for_bit(dtype):
    import torch
    n, E, C = 1024, 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    P, F = len(ia), len(FREQS)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        hc, hp = p.execute_conn(x, out_kind='cross_sum')
        hphi = p.execute_conn(x, out_kind='plv_sum')
        tx = torch.from_numpy(np.array(x)).cuda()
        oc = torch.full((P, F, n), float('nan'), dtype=torch.complex128, device='cuda')
        op = torch.full((C, F, n), float('nan'), dtype=torch.float64, device='cuda')
        ophi = torch.full((P, F, n), float('nan'), dtype=torch.complex128, device='cuda')
        assert p.execute_conn(tx, out=(oc, op), out_kind='cross_sum')[0] is oc
        p.execute_conn(tx, out=ophi, out_kind='plv_sum')
        dev = (oc.cpu().numpy(), op.cpu().numpy(), ophi.cpu().numpy())
        oc2 = torch.full((P, F, n), float('nan'), dtype=torch.complex128, device='cuda')
        p.execute_conn(tx, out=(oc2, None), out_kind='cross_sum')         # no power sums
        dev2 = oc2.cpu().numpy()
        with pytest.raises(ValueError, match='output'):
            p.execute_conn(tx, out_kind='cross_sum')
        with pytest.raises(ValueError, match='complex128'):
            p.execute_conn(tx, out=(op, op), out_kind='cross_sum')
        with pytest.raises(ValueError, match='hold'):
            p.execute_conn(tx, out=(oc[:3], op), out_kind='cross_sum')
        with pytest.raises(ValueError, match='epochs, channels'):
            p.execute_conn(tx.reshape(E * C, n), out=(oc, op), out_kind='cross_sum')
    finally:
        p.close()
    assert np.array_equal(dev[0], hc) and np.array_equal(dev[1], hp) and np.array_equal(dev[2], hphi)
    assert np.array_equal(dev2, hc)


@pytest.mark.parametrize('dtype', DTYPES)
def test_edge_cases_and_errors(dtype):
    n, E, C = 1024, 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    F = len(FREQS)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        full_c, full_p = p.execute_conn(x, out_kind='cross_sum')
        # no epochs: zero sums
        c0, p0 = p.execute_conn(x[:0], out_kind='cross_sum')
        phi0 = p.execute_conn(x[:0], out_kind='plv_sum')
        assert c0.shape == full_c.shape and p0.shape == full_p.shape and phi0.shape == full_c.shape
        assert not np.any(c0) and not np.any(p0) and not np.any(phi0)
        # no pairs: an empty cross, the power sums as ever
        ce, pe = p.execute_conn(x, ([], []), out_kind='cross_sum')
        assert ce.shape == (0, F, n) and np.array_equal(pe, full_p)
        assert p.execute_conn(x, ([], []), out_kind='plv_sum').shape == (0, F, n)
        # PLV forms no power sums
        xc = np.ascontiguousarray(x)
        ia, ib = all_pairs(C)
        V_ = ctypes.c_void_p
        rc = L.lib().nw_execute_conn(p.handle, xc.ctypes.data_as(V_), E, C, ia.ctypes.data_as(V_), ib.ctypes.data_as(V_),
                                     len(ia), full_c.ctypes.data_as(V_), full_p.ctypes.data_as(V_), L.NW_OUT_PLV_SUM,
                                     L.NW_MEM_HOST)
        assert rc == L.NW_E_INVALID and b'out_power must be NULL' in L.lib().nw_last_error()
        with pytest.raises(ValueError, match='out_kind'):
            p.execute_conn(x, out_kind='coherence')
        with pytest.raises(ValueError, match='indices'):
            p.execute_conn(x, ([0], [C]))
    finally:
        p.close()
    small = morse_plan(n, dtype, FREQS, C - 1)
    try:
        with pytest.raises(ValueError, match='max_batch'):
            small.execute_conn(x)
        assert small.execute(x[0, :1], out_kind='power').shape == (1, F, n)      # the plan still works
    finally:
        small.close()


def test_conn_under_bounds_checks():
    """The debug library (kernel bounds checks, nw_dcheck.h) on several pair tiles with partial
    ones (C = 17) and on a tail tile (n = 1201): no check fails."""
    body = ('rng = np.random.default_rng(1)\n'
            'for n, E, C, dt in ((1024, 3, 17, "float64"), (1201, 3, 5, "float32")):\n'
            '    x = rng.standard_normal((E, C, n)).astype(dt)\n'
            '    p = nw.Plan(n, 3, dt, max_batch=2 * C + 3)\n'
            '    p.set_wavelet("morse", [17.5, 3.], np.array([3., 30., 200.]), L.trans_grid(n / 1000., 1000., False))\n'
            '    c, pw = p.execute_conn(x)\n'
            '    phi = p.execute_conn(x, ([C - 1, 0, 2], [0, 0, 2]), out_kind="plv_sum")\n'
            '    print("ok", n, bool(np.all(np.isfinite(c)) and np.all(pw > 0) and np.all(np.isfinite(phi))))\n'
            '    p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok 1024 True' in lines and 'ok 1201 True' in lines, lines
