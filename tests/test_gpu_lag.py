"""GPU tests of phase-lag connectivity: NW_OUT_LAG_SUM through nw_execute_pair (k_accumulate_pair's
lag mode) and nw_execute_conn (nw_conn_accumulate_kernel's lag mode), Plan.execute_pair /
execute_conn, WaveletBase.lag_batch / lag_connectivity_batch and EpochsWavelet.

For epochs e, channels c with rows y_e,c (F, n_out), a pair (a, b) and m_e = Im y_a,e conj(y_b,e):
    L0 = sum_e m_e,  L1 = sum_e |m_e|,  L2 = sum_e m_e^2,  L3 = sum_e sgn m_e
every sum in fp64 in epoch order.  References are formed here from oracle.nw_oracle in complex128.

Inputs: the lagged recipe of epoch_cases.py, test_gpu_conn.py's with a lag, so that the sign sums are not centred
on 0: rng = default_rng(2300 + n), common = rng.standard_normal((E, 1, n)), noise = rng.standard_normal((E, C, n)),
x[:, c] = 0.6 roll(common[:, 0], 3 c) + 0.8 noise[:, c]; Morse(1000) with its default b, r and the nine
scales FREQS (three, FREQS3, where stated).

Bounds.  A_e,c: that signal's max|y| over (F, N) of the undecimated rows; S = sum_e A_e,a A_e,b;
tol: 1e-12 fp64, 1e-5 fp32, 2e-5 fp32 on chirp-z lengths (the per-signal contract).
  T1  against the oracle, pointwise: |dL0|, |dL1| <= 2 tol S (a row error tol A on each factor moves
      m_e by at most 2 tol A_a A_b, and ||u| - |v|| <= |u - v|); |dL2| <= 5 tol sum_e (A_e,a A_e,b)^2
      (4 tol (1 + tol) and room for the fp64 additions); L3 exactly equal at the visible points, where
      every epoch has |m_e| >= v A_e,a A_e,b with v = 1e-4 fp32 (2.5 x the largest perturbation 2 tol
      at the chirp tolerance: no sign can flip) / 1e-9 fp64; at least 0.8 of every pair's points are
      visible (0.6 for the 17-channel three-scale case), asserted on the reference alone
  T2  against the same plan's own rows reduced in numpy complex128 in epoch order: |dL0|, |dL1| <=
      1e-13 sum |y_a||y_b|, |dL2| <= 1e-13 sum (|y_a||y_b|)^2, L3 exactly equal where every epoch has
      |m_e| >= 1e-12 |y_a||y_b| (at least 0.8 of the points)
  T3  w = 0.003: where the reference has L1 >= w S (at least 0.55 of every pair's points, asserted on
      the reference alone) |dwpli| <= 4.1 tol / w, from (|dL0| + wpli |dL1|) / L1_device with
      L1_device >= (w - 2 tol) S; pli and dpli exactly equal where every epoch is visible
The exact comparisons between differently chunked calls are made in fp64, where a row depends on its
signal alone (test_gpu_conn.py)."""
import ctypes

import numpy as np
import pytest

from epoch_cases import (EPOCH_AXIS, FREQS, SHAPES, FakeEpochs, forms, morse_plan, run_under_bounds_checks, tol_of,
                         vis_of)
from epoch_cases import lagged_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import LAG_OUTS, all_pairs, finalize_lag  # noqa: E402

W = 0.003
DTYPES = ['float32', 'float64']
LAG_NAMES = ['pli', 'pli2_unbiased', 'dpli', 'wpli', 'wpli2_debiased']


def lag_of(y, ia, ib, floor, scale=None):
    """(sums (P, F, n, 4), seen (P, F, n)) of complex128 rows (E, C, F, n), added in epoch order; seen:
    every epoch has |m_e| >= floor * scale[e] (scale (E, P) or, None, |y_a||y_b| pointwise)."""
    sums = np.zeros((len(ia),) + y.shape[2:] + (4,))
    seen = np.ones((len(ia),) + y.shape[2:], dtype=bool)
    for e in range(y.shape[0]):
        a, b = y[e][ia], y[e][ib]
        m = a.imag * b.real - a.real * b.imag
        sums[..., 0] += m
        sums[..., 1] += np.abs(m)
        sums[..., 2] += m * m
        sums[..., 3] += np.sign(m)
        seen &= np.abs(m) >= floor * (np.abs(a) * np.abs(b) if scale is None else scale[e][:, None, None])
    return sums, seen


def run_lag(n, dtype, freqs, max_batch, x, indices=None, **kw):
    """(lag sums, stats) of one plan."""
    p = morse_plan(n, dtype, freqs, max_batch, **kw)
    try:
        return p.execute_conn(x, indices, out_kind='lag_sum'), p.stats()
    finally:
        p.close()


def check_t1(name, got, y, A, ia, ib, tol, dtype, share=0.8):
    """T1 of lag sums ``got`` (P, F, n', 4) for the pairs (ia, ib) against the reference rows y (E, C, F, n')
    with A (E, C) the row scales."""
    AB = A[:, ia] * A[:, ib]                                  # (E, P)
    want, seen = lag_of(y, ia, ib, vis_of(dtype), AB)
    per_pair = seen.mean(axis=(1, 2))
    assert np.all(per_pair >= share), (name, per_pair.min())  # on the reference alone
    S = np.sum(AB, axis=0)[:, None, None]
    S2 = np.sum(AB * AB, axis=0)[:, None, None]
    d = np.abs(got - want)
    e0, e1, e2 = np.max(d[..., 0] / S), np.max(d[..., 1] / S), np.max(d[..., 2] / S2)
    flips = int(np.count_nonzero(got[..., 3][seen] != want[..., 3][seen]))
    print(f'{name} T1: dL0 {e0 / (2 * tol):.3f} dL1 {e1 / (2 * tol):.3f} dL2 {e2 / (5 * tol):.3f} of the bound '
          f'(tol {tol:.0e}); visible {per_pair.min():.2f}-{per_pair.max():.2f} per pair, {flips} sign sums differ there')
    assert e0 <= 2 * tol and e1 <= 2 * tol and e2 <= 5 * tol, (name, e0, e1, e2)
    assert flips == 0, (name, flips)
    assert np.array_equal(got[..., 3], np.rint(got[..., 3])), name     # L3 holds integers
    return want, seen


# (id, n, dtype, E, C, freqs, plan keywords, decim, kernel of the form, visible share): five epochs but for the rows
# of SHAPES
CASES = []
for name, n, dtype, kw, decim, _, kernel in forms(*EPOCH_AXIS):
    E, C, freqs = SHAPES.get(name, (5, 5, FREQS))
    CASES.append((name, n, dtype, E, C, freqs, kw, decim, kernel, 0.6 if name == 'tiles-17ch-f64' else 0.8))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_lag_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 and T2 for every pair a < b through nw_execute_conn, T1 for one pair through
    nw_execute_pair; max_batch = 2 C + 3: uneven chunks and a batch that is no multiple of C."""
    name, n, dtype, E, C, freqs, kw, decim, kernel, share = case
    x, y = oracle_rows(n, E, C, dtype, freqs)
    A = np.max(np.abs(y), axis=(2, 3))                       # (E, C), of the undecimated rows
    y = y[..., ::decim]
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        lag = p.execute_conn(x, out_kind='lag_sum')
        st = p.stats()
        a, b = 0, C - 1
        pair = p.execute_pair(x[:, a], x[:, b], out_kind='lag_sum')
        st_pair = p.stats()
        rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape((E, C) + y.shape[2:])
    finally:
        p.close()
    P, F, no = len(ia), len(freqs), n // decim
    assert lag.shape == (P, F, no, 4) and lag.dtype == np.float64
    assert pair.shape == (F, no, 4) and pair.dtype == np.float64
    assert st['reduce_path'] == L.NW_REDUCE_CONN and st_pair['reduce_path'] == L.NW_REDUCE_ROWS, (name, st, st_pair)
    assert L.KERNEL_NAMES[st['kernel']] == kernel and L.KERNEL_NAMES[st_pair['kernel']] == kernel, (name, st, st_pair)
    assert st['chunks'] == -(-E // 2), (name, st)
    if C > 16:
        assert L.conn_tiles(C, ia, ib)[1] == 3
    # T1
    check_t1(name, lag, y, A, ia, ib, tol, dtype, share)
    check_t1(name + ' pair', pair[None], y, A, np.array([a]), np.array([b]), tol, dtype, share)
    # T2
    own, near = lag_of(rows, ia, ib, 1e-12)
    mag = np.abs(rows)
    sab = np.zeros((P, F, no))
    sab2 = np.zeros((P, F, no))
    for e in range(E):
        ab = mag[e][ia] * mag[e][ib]
        sab += ab
        sab2 += ab * ab
    d = np.abs(lag - own)
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = [np.nanmax(np.where(sab > 0, d[..., 0] / sab, 0)), np.nanmax(np.where(sab > 0, d[..., 1] / sab, 0)),
                 np.nanmax(np.where(sab2 > 0, d[..., 2] / sab2, 0))]
    flips = int(np.count_nonzero(lag[..., 3][near] != own[..., 3][near]))
    print(f'{name} T2: dL0 {worst[0]:.2e} dL1 {worst[1]:.2e} dL2 {worst[2]:.2e} (bound 1e-13); '
          f'{near.mean():.3f} of the points have every |m| >= 1e-12 |y_a||y_b|, {flips} sign sums differ there')
    assert np.all(d[..., 0] <= 1e-13 * sab) and np.all(d[..., 1] <= 1e-13 * sab), (name, worst)
    assert np.all(d[..., 2] <= 1e-13 * sab2), (name, worst)
    assert near.mean() >= 0.8 and flips == 0, (name, near.mean(), flips)


T3_CASES = [(1024, 5, 5, FREQS), (1201, 5, 5, FREQS), (1024, 3, 17, FREQS), (4096, 5, 5, FREQS)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', T3_CASES, ids=[f'{n}-{E}x{C}' for n, E, C, _ in T3_CASES])
def test_wpli_pli_and_dpli_on_visible_points(shape, dtype):
    """T3 for every pair."""
    n, E, C, freqs = shape
    x, y = oracle_rows(n, E, C, dtype, freqs)
    ia, ib = all_pairs(C)
    tol = tol_of(n, dtype)
    A = np.max(np.abs(y), axis=(2, 3))
    AB = A[:, ia] * A[:, ib]
    want, seen = lag_of(y, ia, ib, vis_of(dtype), AB)
    S = np.sum(AB, axis=0)[:, None, None]
    heavy = want[..., 1] >= W * S
    per_pair = heavy.mean(axis=(1, 2))
    assert np.all(per_pair >= 0.55), per_pair.min()          # on the reference alone
    lag, _ = run_lag(n, dtype, freqs, 2 * C + 3, x)
    dw = np.abs(finalize_lag('wpli', lag, E) - finalize_lag('wpli', want, E))
    worst = np.max(dw[heavy])
    print(f'n={n} E={E} C={C} {dtype} T3: L1 >= w S at {per_pair.min():.2f}-{per_pair.max():.2f} of the points per '
          f'pair; dwpli {worst:.3e} = {worst / (4.1 * tol / W):.4f} of the bound; every epoch visible at '
          f'{seen.mean(axis=(1, 2)).min():.2f}')
    assert worst <= 4.1 * tol / W
    for kind in ('pli', 'dpli'):
        assert np.array_equal(finalize_lag(kind, lag, E)[seen], finalize_lag(kind, want, E)[seen]), kind


@pytest.mark.parametrize('n', [1024, 1201])
def test_bit_identities(n):
    """fp64: L0 is the imaginary part of the cross sums (conn and the pair's rows path), the conn lag
    sums of a pair are nw_execute_pair's, and chunking changes nothing."""
    dtype, E, C = 'float64', 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        lag = p.execute_conn(x, out_kind='lag_sum')
        cross, _ = p.execute_conn(x, out_kind='cross_sum')
        assert np.array_equal(lag[..., 0], cross.imag)
        for a, b in ((0, 3), (2, 4)):
            k = int(np.flatnonzero((ia == a) & (ib == b))[0])
            sums = p.execute_pair(x[:, a], x[:, b], out_kind='cross_sum')
            assert p.stats()['reduce_path'] == L.NW_REDUCE_ROWS
            pair = p.execute_pair(x[:, a], x[:, b], out_kind='lag_sum')
            assert p.stats()['reduce_path'] == L.NW_REDUCE_ROWS
            assert np.array_equal(lag[k, ..., 0], sums[..., 1]), (a, b)
            assert np.array_equal(lag[k], pair), (a, b)
    finally:
        p.close()
    one, st_one = run_lag(n, dtype, FREQS, C, x)
    all_, st_all = run_lag(n, dtype, FREQS, E * C, x)
    assert st_one['chunks'] == E and st_all['chunks'] == 1
    assert np.array_equal(one, all_) and np.array_equal(one, lag)


@pytest.mark.parametrize('dtype', DTYPES)
def test_indexed_list_with_reversed_repeated_and_self_pairs(dtype):
    n, E, C = 1024, 5, 6
    x, y = oracle_rows(n, E, C, dtype, FREQS)
    ia = np.array([5, 0, 3, 3, 0, 2])
    ib = np.array([0, 5, 3, 1, 5, 2])
    lag, st = run_lag(n, dtype, FREQS, 2 * C + 3, x, (ia, ib))
    assert st['reduce_path'] == L.NW_REDUCE_CONN and lag.shape == (6, len(FREQS), n, 4)
    # results land in the caller's order: T1 against the oracle for this list (the self pairs have no
    # visible point: their sums are compared below)
    A = np.max(np.abs(y), axis=(2, 3))
    real = np.flatnonzero(ia != ib)
    check_t1(f'list {dtype}', lag[real], y, A, ia[real], ib[real], tol_of(n, dtype), dtype)
    # (5, 0) against (0, 5): L0 and L3 negated, L1 and L2 equal, exactly; (0, 5) twice: equal
    assert np.array_equal(lag[0, ..., 0], -lag[1, ..., 0]) and np.array_equal(lag[0, ..., 3], -lag[1, ..., 3])
    assert np.array_equal(lag[0, ..., 1], lag[1, ..., 1]) and np.array_equal(lag[0, ..., 2], lag[1, ..., 2])
    assert np.any(lag[1, ..., 3])
    assert np.array_equal(lag[1], lag[4])
    # the self pairs (3, 3) and (2, 2): four exact zeros
    for k in (2, 5):
        assert not np.any(lag[k])
        assert not np.any(finalize_lag('wpli', lag[k], E)) and not np.any(finalize_lag('pli', lag[k], E))
        assert np.array_equal(finalize_lag('dpli', lag[k], E), np.full(lag[k].shape[:-1], 0.5))


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_tensors_equal_the_host_call_bit_for_bit(dtype):
    import torch
    n, E, C = 1024, 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    P, F = len(ia), len(FREQS)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        host = p.execute_conn(x, out_kind='lag_sum')
        host_pair = p.execute_pair(x[:, 1], x[:, 3], out_kind='lag_sum')
        tx = torch.from_numpy(np.array(x)).cuda()
        ta, tb = tx[:, 1].contiguous(), tx[:, 3].contiguous()
        out = torch.full((P, F, n, 4), float('nan'), dtype=torch.float64, device='cuda')
        out_pair = torch.full((F, n, 4), float('nan'), dtype=torch.float64, device='cuda')
        assert p.execute_conn(tx, out=out, out_kind='lag_sum') is out
        assert p.execute_pair(ta, tb, out=out_pair, out_kind='lag_sum') is out_pair
        dev, dev_pair = out.cpu().numpy(), out_pair.cpu().numpy()
        wrong = torch.zeros((P, F, n, 2), dtype=torch.complex128, device='cuda')
        with pytest.raises(ValueError, match='output'):
            p.execute_conn(tx, out_kind='lag_sum')
        with pytest.raises(ValueError, match='float64'):
            p.execute_conn(tx, out=wrong, out_kind='lag_sum')
        with pytest.raises(ValueError, match='hold'):
            p.execute_conn(tx, out=out[:3], out_kind='lag_sum')
        with pytest.raises(ValueError, match='epochs, channels'):
            p.execute_conn(tx.reshape(E * C, n), out=out, out_kind='lag_sum')
        with pytest.raises(ValueError, match='output'):
            p.execute_pair(ta, tb, out_kind='lag_sum')
        with pytest.raises(ValueError, match='float64'):
            p.execute_pair(ta, tb, out=wrong, out_kind='lag_sum')
        with pytest.raises(ValueError, match='contiguous'):
            p.execute_pair(ta, tb, out=out_pair[:3], out_kind='lag_sum')
        with pytest.raises(ValueError, match='out_kind'):
            p.execute_pair(ta, tb, out=out_pair, out_kind='wpli')
        with pytest.raises(ValueError, match='out_kind'):
            p.execute_conn(tx, out=out, out_kind='wpli')
    finally:
        p.close()
    assert np.array_equal(dev, host) and np.array_equal(dev_pair, host_pair)


@pytest.mark.parametrize('dtype', DTYPES)
def test_edge_cases_and_errors(dtype):
    n, E, C = 1024, 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    F = len(FREQS)
    ia, ib = all_pairs(C)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        full = p.execute_conn(x, out_kind='lag_sum')
        # no epochs: zero sums
        none = p.execute_conn(x[:0], out_kind='lag_sum')
        assert none.shape == full.shape and not np.any(none)
        none_pair = p.execute_pair(x[:0, 0], x[:0, 1], out_kind='lag_sum')
        assert none_pair.shape == (F, n, 4) and not np.any(none_pair)
        # no pairs: an empty result
        assert p.execute_conn(x, ([], []), out_kind='lag_sum').shape == (0, F, n, 4)
        # the lag sums carry no power sums
        xc = np.ascontiguousarray(x)
        power = np.empty((C, F, n))
        V_ = ctypes.c_void_p
        rc = L.lib().nw_execute_conn(p.handle, xc.ctypes.data_as(V_), E, C, ia.ctypes.data_as(V_), ib.ctypes.data_as(V_),
                                     len(ia), full.ctypes.data_as(V_), power.ctypes.data_as(V_), L.NW_OUT_LAG_SUM,
                                     L.NW_MEM_HOST)
        assert rc == L.NW_E_INVALID and b'out_power must be NULL' in L.lib().nw_last_error()
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_conn(x, out=np.empty((len(ia), F, n), dtype=np.complex128), out_kind='lag_sum')
        with pytest.raises(ValueError, match='indices'):
            p.execute_conn(x, ([0], [C]), out_kind='lag_sum')
        assert np.array_equal(p.execute_conn(x, out_kind='lag_sum'), full)          # the plan still works
    finally:
        p.close()


def test_class_layer():
    """Every finalised output is finalize_lag of the same call's own sums, exactly; one plan; decim;
    EpochsWavelet."""
    dtype, n, E, C = 'float64', 1024, 5, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ia, ib = all_pairs(C)
    w = nw.Morse(1000, dtype=dtype)
    got = {out: w.lag_connectivity_batch(x, FREQS, out=out) for out in LAG_OUTS}
    assert len(w._plans) == 1 and w.plan_stats()[0]['reduce_path'] == L.NW_REDUCE_CONN
    sums = got['lag_sum']
    assert sums.shape == (len(ia), len(FREQS), n, 4) and sums.dtype == np.float64
    phi = w.connectivity_batch(x, FREQS, out='plv_sum')      # the existing path's unit-phasor sums
    assert len(w._plans) == 1
    for out in LAG_OUTS:
        if out == 'lag_sum':
            continue
        assert got[out].shape == (len(ia), len(FREQS), n) and got[out].dtype == np.float64, out
        assert np.array_equal(got[out], finalize_lag(out, phi if LAG_OUTS[out] == 'plv_sum' else sums, E)), out
    assert np.all(got['wpli'] <= 1) and np.all(got['pli'] <= 1) and np.all(np.abs(got['dpli'] - 0.5) <= 0.5)
    # two channels: lag_batch, pair by pair the conn sums exactly (fp64)
    wp = nw.Morse(1000, dtype=dtype)
    for k, (a, b) in enumerate(zip(ia, ib)):
        if (a, b) not in ((0, 3), (2, 4)):
            continue
        pair = {out: wp.lag_batch(x[:, a], x[:, b], FREQS, out=out) for out in LAG_OUTS}
        assert np.array_equal(pair['lag_sum'], sums[k]), (a, b)
        plv_sum = wp.cross_batch(x[:, a], x[:, b], FREQS, out='plv_sum')
        for out in LAG_OUTS:
            src = plv_sum if LAG_OUTS[out] == 'plv_sum' else pair['lag_sum']
            assert np.array_equal(pair[out], finalize_lag(out, src, E)), (out, a, b)
            assert pair[out].shape == ((len(FREQS), n, 4) if out == 'lag_sum' else (len(FREQS), n)), out
    assert wp.plan_stats()[0]['reduce_path'] == L.NW_REDUCE_ROWS
    # an index list, and EpochsWavelet: positions in ch_names, channels picked from the epochs
    idx = ([2, 0], [0, 1])
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)          # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype))
    sub = np.ascontiguousarray(x[:, :3])
    for method in ('wpli', 'pli', 'dpli', 'wpli2_debiased', 'ciplv', 'ppc', 'pli2_unbiased', 'lag_sum'):
        assert np.array_equal(ew.lag_connectivity(['a', 'b', 'c'], FREQS, method=method),
                              w.lag_connectivity_batch(sub, FREQS, out=method)), method
        assert np.array_equal(ew.lag_connectivity(['a', 'b', 'c'], FREQS, method=method, indices=idx),
                              w.lag_connectivity_batch(sub, FREQS, out=method, indices=idx)), method
    own = wp.lag_batch(x[:, 0], x[:, 1], FREQS, out='lag_sum')              # channels 'a' and 'b'
    own_phi = wp.cross_batch(x[:, 0], x[:, 1], FREQS, out='plv_sum')
    for name in ('pli', 'dpli', 'wpli', 'wpli2_debiased', 'ciplv'):
        src = own_phi if LAG_OUTS[name] == 'plv_sum' else own
        assert np.array_equal(getattr(ew, name)('a', 'b', FREQS), finalize_lag(name, src, E)), name
    # decim: n = 1201 has no device decimation: the undecimated result [..., ::5], exactly
    x5, _ = oracle_rows(1201, E, C, dtype, FREQS)
    w5 = nw.Morse(1000, dtype=dtype)
    for out in ('wpli', 'dpli', 'wpli2_debiased', 'ciplv'):
        full = w5.lag_connectivity_batch(x5, FREQS, out=out)
        dec = w5.lag_connectivity_batch(x5, FREQS, out=out, decim=5)
        assert dec.shape == (len(ia), len(FREQS), 241) and np.array_equal(dec, full[..., ::5]), out
        full = w5.lag_batch(x5[:, 0], x5[:, 1], FREQS, out=out)
        dec = w5.lag_batch(x5[:, 0], x5[:, 1], FREQS, out=out, decim=5)
        assert dec.shape == (len(FREQS), 241) and np.array_equal(dec, full[..., ::5]), out
    fs = w5.lag_connectivity_batch(x5, FREQS, out='lag_sum')
    ds = w5.lag_connectivity_batch(x5, FREQS, out='lag_sum', decim=5)
    assert ds.shape == (len(ia), len(FREQS), 241, 4) and np.array_equal(ds, fs[:, :, ::5])
    # ... and on the device where supported (n = 4096, decim 4)
    x4, y4 = oracle_rows(4096, E, C, 'float32', FREQS)
    w4 = nw.Morse(1000, dtype='float32')
    s4 = w4.lag_connectivity_batch(x4, FREQS, out='lag_sum', decim=4)
    assert s4.shape == (len(ia), len(FREQS), 1024, 4)
    assert L.KERNEL_NAMES[w4.plan_stats()[0]['kernel']] == 'nw_fused_decim_kernel'
    check_t1('class decim-4096', s4, y4[..., ::4], np.max(np.abs(y4), axis=(2, 3)), ia, ib, 1e-5, 'float32')
    assert np.array_equal(w4.lag_connectivity_batch(x4, FREQS, out='wpli', decim=4), finalize_lag('wpli', s4, E))


def test_lag_under_bounds_checks():
    """The debug library (kernel bounds checks, nw_dcheck.h) on several pair tiles with partial
    ones (C = 17) and on a tail tile (n = 1201), with a short index list and through the pair path:
    no check fails."""
    body = ('rng = np.random.default_rng(1)\n'
            'for n, E, C, dt in ((1024, 3, 17, "float64"), (1201, 3, 5, "float32")):\n'
            '    x = rng.standard_normal((E, C, n)).astype(dt)\n'
            '    p = nw.Plan(n, 3, dt, max_batch=2 * C + 3)\n'
            '    p.set_wavelet("morse", [17.5, 3.], np.array([3., 30., 200.]), L.trans_grid(n / 1000., 1000., False))\n'
            '    full = p.execute_conn(x, out_kind="lag_sum")\n'
            '    short = p.execute_conn(x, ([C - 1, 0, 2], [0, 0, 2]), out_kind="lag_sum")\n'
            '    pair = p.execute_pair(x[:, 0], x[:, C - 1], out_kind="lag_sum")\n'
            '    ok = all(bool(np.all(np.isfinite(a))) for a in (full, short, pair))\n'
            '    print("ok", n, ok and full.shape == (C * (C - 1) // 2, 3, n, 4) and short.shape == (3, 3, n, 4))\n'
            '    p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok 1024 True' in lines and 'ok 1201 True' in lines, lines
