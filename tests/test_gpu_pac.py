"""GPU tests of phase-amplitude coupling: nw_execute_pac (nw_pac_kernel and nw_pac_rows_kernel, nw_pac.hip)
through Plan.execute_pac, engine.finalize_pac, WaveletBase.pac_batch and EpochsWavelet.pac.

For epoch e, a pair (p, a) of a phase and an amplitude channel with rows y_e,c (F, n_out), listed phase scales
fph, amplitude scales fam and a window of T samples s_j = t0 + j step, with A = |y_a[fa, s_j]| and
u = y_p[fp, s_j] / |y_p[fp, s_j]|:
    M = sum_j A u (E, P, Fp, Fa),  amp = {sum_j A, sum_j A^2} (E, C, Fa, 2),  phase = sum_j u (E, C, Fp).
References are formed here from oracle.nw_oracle in complex128.

Inputs: the coupled recipe of epoch_cases.py: rng = default_rng(2600 + n); x[:, c] = 0.6 roll(common, 3 c) +
0.8 noise[:, c] (the lagged recipe on another seed); every even channel also gets 2 cos(phi) + 1.5 (1 + 0.9 cos(phi)) cos(2 pi 70 t + 1), phi = 2 pi 7 t + a uniform
random phase per epoch: a 70 Hz amplitude that follows the 7 Hz phase.  sfreq 1000, Morse(1000) with its default
b, r, FREQS (nine scales), phase = [0, 1, 2, 3], amp = [4 .. 8], E = 3, C = 5, max_batch = 2 C + 3 (chunks of 2 and
1 epochs) unless stated.  PAIRS: every channel with itself and three cross-channel pairs.
Windows (the plan's output samples): full, (0, 1), (37, 1001), an empty one and a stride-4 one; the full-rate
n = 1000 plan of the rocFFT case takes them through engine.time_window with decim = 4 (its step-4 path).

tol: 1e-12 fp64, 1e-5 fp32, 2e-5 fp32 on chirp-z lengths; A_c: the signal's max |y| over (F, N) of its undecimated
rows; u_j = min(2, 2 tol A_p / |y_p|) (a unit phasor moves by at most 2 |dy| / |y|).
  T1  against the oracle: |dM| <= sum_j [2 tol A_a (1 + u_j) + |y_a| u_j] + 1e-13 T A_a; |d sum A| <= 2 tol T A_c;
      |d sum A^2| <= 2 (2 tol) T A_c^2; |d sum u| <= sum_j u_j + 1e-13 T.  On the reference alone, at n = 1024 and
      n = 1201 for the windows full and (37, 1001): sum_j u_j <= 0.02 T at every scale; sqrt(T sum A^2) / (T A_c)
      >= 0.05; in the epoch-averaged direct_pac the coupled cell (7 Hz, 70 Hz) of every even channel is >= 2 x the
      largest cell of the uncoupled channel (UNCOUPLED).
  T2  fp64: the same plan's own rows reduced in numpy in the contract's order: sum A^2 array_equal; M, sum A and
      sum u within 1e-13 T (A_a, A_c, 1) (hypot and the division may differ in the last place).
  T3  bit for bit, fp32 and fp64: amp[..., 1] is execute_conn_time's power; a pair's M under any pair list, any
      phase / amp lists, any max_batch, device tensors.
  T4  measures: fp64 every kind within 1e-7 of the formula on the oracle's sums; fp32 |d direct_pac| <=
      (bM + 2 tol T A_a) / (sqrt(T sum A^2) - 2 tol T A_a) on every cell, bM the T1 bound.
  T5  the layers; T6 the debug library."""
import numpy as np
import pytest

from epoch_cases import (FREQS, OVER_TIME, FakeEpochs, forms, lane_sum, morse_plan, run_under_bounds_checks, tol_of,
                         windows_of)
from epoch_cases import coupled_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import finalize_pac, time_window  # noqa: E402

PHASE, AMP = [0, 1, 2, 3], [4, 5, 6, 7, 8]
FREQS3 = [7., 70., 200.]             # this file's three: the coupled pair of scales is among them
FREQS26 = [float(f) for f in np.round(np.geomspace(4., 300., 26), 2)]
KINDS = ('mvl', 'mvl_norm', 'direct_pac', 'debiased_pac')
# (phase channel, amplitude channel): every channel with itself, then three cross-channel pairs
PAIRS = (np.array([0, 1, 2, 3, 4, 0, 1, 2]), np.array([0, 1, 2, 3, 4, 2, 0, 3]))
# The uncoupled channel of the planted-coupling check.  On the oracle, the epoch-averaged direct_pac of the coupled
# cell is 0.28 .. 0.30 on channels 0, 2, 4; channel 3's largest cell is 0.075 .. 0.130 over the four (n, window)
# checked and channel 1's 0.100 .. 0.143 (its largest, 4 Hz x 40 Hz at n = 1024, (37, 1001), is noise in a window
# of four cycles): 2 x holds against channel 3 everywhere and misses against channel 1 in that one window by 1 %.
UNCOUPLED = 3


def pairs_of(C):
    ip, ia = PAIRS
    keep = (ip < C) & (ia < C)
    return ip[keep], ia[keep]


def ref_sums(y, ip, ia, fph, fam, idx):
    """The oracle's sums over the samples ``idx`` of rows y (E, C, F, n): (M, amp, phase, |y_amp| (E, C, Fa, T),
    |y_phase| (E, C, Fp, T))."""
    yw = y[..., idx]
    ya, yp = yw[:, :, fam], yw[:, :, fph]
    A, mp = np.abs(ya), np.abs(yp)
    with np.errstate(invalid='ignore', divide='ignore'):
        u = yp / mp
    M = np.einsum('epit,epkt->epik', u[:, ip], A[:, ia].astype(np.complex128))
    amp = np.stack([A.sum(-1), (ya.real ** 2 + ya.imag ** 2).sum(-1)], axis=-1)
    return M, amp, u.sum(-1), A, mp


def t1_bounds(A, mp, Ac, ip, ia, tol):
    """(bM (E, P, Fp, Fa), bu (E, C, Fp)): the T1 bounds of M and of sum u; bu without its 1e-13 T."""
    T = A.shape[-1]
    with np.errstate(divide='ignore'):
        u = np.minimum(2., 2 * tol * Ac[:, :, None, None] / mp)                  # (E, C, Fp, T)
    bu = u.sum(-1)
    Aa = Ac[:, ia][:, :, None, None]
    bM = (2 * tol * Aa * (T + bu[:, ip][:, :, :, None]) + np.einsum('epkt,epit->epik', A[:, ia], u[:, ip])
          + 1e-13 * T * Aa)
    return bM, bu


def check_reference(name, y, fph, fam, idx, Ac, tol):
    """On the reference alone: the phasor bound, the denominator of direct_pac and the planted coupling."""
    T = len(idx)
    C = y.shape[1]
    own = np.arange(C)
    M, amp, phase, A, mp = ref_sums(y, own, own, fph, fam, idx)
    _, bu = t1_bounds(A, mp, Ac, own, own, tol)
    den = np.sqrt(T * amp[..., 1]) / (T * Ac[:, :, None])
    pac = finalize_pac('direct_pac', M, amp, phase, own, own, T).mean(axis=0)      # the comodulograms (C, Fp, Fa)
    coupled = pac[0::2, fph.index(1), fam.index(5)]
    print(f'{name} T={T}: reference: phasor bound <= {bu.max() / T:.4f} T, sqrt(T sum A^2) / (T A_c) >= {den.min():.3f}, '
          f'coupled cell {coupled.min():.3f} .. {coupled.max():.3f}, channel {UNCOUPLED} <= {pac[UNCOUPLED].max():.3f} '
          f'(channel 1 <= {pac[1].max():.3f})')
    assert np.all(bu <= 0.02 * T), (name, bu.max() / T)
    assert np.all(den >= 0.05), (name, den.min())
    assert coupled.min() >= 2 * pac[UNCOUPLED].max(), (name, coupled.min(), pac[UNCOUPLED].max())


def check_t1(name, got, y, Ac, ip, ia, fph, fam, idx, tol):
    """T1 of (M, amp, phase) over the window samples ``idx`` (indices into the reference rows)."""
    M, amp, phase = got
    T = len(idx)
    rM, ramp, rphase, A, mp = ref_sums(y, ip, ia, fph, fam, idx)
    assert M.shape == rM.shape and amp.shape == ramp.shape and phase.shape == rphase.shape, name
    bM, bu = t1_bounds(A, mp, Ac, ip, ia, tol)
    dM = np.abs(M - rM)
    dA = np.abs(amp[..., 0] - ramp[..., 0]) / (T * Ac[:, :, None])
    dA2 = np.abs(amp[..., 1] - ramp[..., 1]) / (T * Ac[:, :, None] ** 2)
    du = np.abs(phase - rphase)
    print(f'{name} T1: dM {np.max(dM / bM):.3f} of its bound, d sum A {dA.max() / (2 * tol):.3f}, d sum A^2 '
          f'{dA2.max() / (4 * tol):.3f} of the bound (tol {tol:.0e}); d sum u {np.max(du - bu - 1e-13 * T):.3e} over its bound')
    assert np.all(dM <= bM), (name, np.max(dM / bM))
    assert dA.max() <= 2 * tol and dA2.max() <= 4 * tol, (name, dA.max(), dA2.max())
    assert np.all(du <= bu + 1e-13 * T), name
    return rM, ramp, rphase, bM


def own_sums(rows, ip, ia, fph, fam, idx):
    """(M, amp, phase) of the plan's own complex128 rows (E, C, F, n_out) in the contract's order."""
    yw = rows[..., idx]
    re, im = np.ascontiguousarray(yw.real), np.ascontiguousarray(yw.imag)
    A = np.hypot(re[:, :, fam], im[:, :, fam])                                    # (E, C, Fa, T)
    p1, p2 = re[:, :, fam] * re[:, :, fam], im[:, :, fam] * im[:, :, fam]
    amp = np.stack([lane_sum(A), lane_sum(p1 + p2)], axis=-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        h = np.hypot(re[:, :, fph], im[:, :, fph])
        ur, ui = re[:, :, fph] / h, im[:, :, fph] / h                             # (E, C, Fp, T)
    phase = lane_sum(ur) + 1j * lane_sum(ui)
    Aa = A[:, ia][:, :, None]                                                     # (E, P, 1, Fa, T)
    M = lane_sum(Aa * ur[:, ip][:, :, :, None]) + 1j * lane_sum(Aa * ui[:, ip][:, :, :, None])
    return M, amp, phase


# (id, n, dtype, E, C, freqs, phase, amp, plan keywords, device decim, host decim, kernel of the form): three epochs
# of five channels, PHASE and AMP of the nine scales, but for the two-pass row; the tile row is this file's own
CASES = []
for name, n, dtype, kw, decim, host_decim, kernel in forms(*OVER_TIME[:-1]):
    E, C, freqs, fph, fam = (2, 3, FREQS3, [0], [1, 2]) if name == 'twopass-32768' else (3, 5, FREQS, PHASE, AMP)
    CASES.append((name, n, dtype, E, C, freqs, fph, fam, kw, decim, host_decim, kernel))
# 9 phase x 17 amplitude scales: two phase tiles and two amplitude tiles, one of each partial
CASES.append(('tiles-9x17-f64', 1024, 'float64', 2, 2, FREQS26, list(range(9)), list(range(9, 26)), {}, 1, 1,
              'nw_fused_kernel'))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 for every case and window, T2 for the fp64 cases; PAIRS; max_batch = 2 C + 3."""
    name, n, dtype, E, C, freqs, fph, fam, kw, decim, host_decim, kernel = case
    x, y = oracle_rows(n, E, C, dtype, freqs)
    Ac = np.max(np.abs(y), axis=(2, 3))                       # (E, C), of the undecimated rows
    ip, ia = pairs_of(C)
    tol = tol_of(n, dtype)
    n_out = n // decim
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        assert p.n_out == n_out
        got = {}
        for wname, win, step in windows_of(n, n_out, host_decim):
            got[wname] = (win, step, p.execute_pac(x, (ip, ia), fph, fam, win, step))
            st = p.stats()
            assert st['reduce_path'] == L.NW_REDUCE_PAC and L.KERNEL_NAMES[st['kernel']] == kernel, (name, st)
        assert st['chunks'] == len(got) * -(-E // ((2 * C + 3) // C)), (name, st)
        rows = None
        if dtype == 'float64':
            rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, len(freqs), n_out)
    finally:
        p.close()
    for wname, (win, step, sums) in got.items():
        idx = np.arange(win[0], win[1], step)
        T = len(idx)
        assert T == L.conn_time_count(n_out, win[0], win[1], step)
        M, amp, phase = sums
        assert M.dtype == np.complex128 and amp.dtype == np.float64 and phase.dtype == np.complex128
        assert M.shape == (E, len(ip), len(fph), len(fam)) and amp.shape == (E, C, len(fam), 2)
        assert phase.shape == (E, C, len(fph))
        if T == 0:                                             # an empty window: zero sums
            assert not np.any(M) and not np.any(amp) and not np.any(phase), (name, wname)
            continue
        if n in (1024, 1201) and freqs is FREQS and wname in ('full', 'inner'):
            check_reference(f'{name} {wname}', y, fph, fam, idx, Ac, tol)
        check_t1(f'{name} {wname}', sums, y, Ac, ip, ia, fph, fam, idx * decim, tol)
        if rows is not None:                                   # T2
            oM, oamp, ophase = own_sums(rows, ip, ia, fph, fam, idx)
            assert np.array_equal(amp[..., 1], oamp[..., 1]), (name, wname, np.abs(amp - oamp)[..., 1].max())
            dM = np.max(np.abs(M - oM) / Ac[:, ia][:, :, None, None])
            dA = np.max(np.abs(amp[..., 0] - oamp[..., 0]) / Ac[:, :, None])
            du = np.abs(phase - ophase).max()
            print(f'{name} {wname} T2: sum A^2 equal bit for bit; dM {dM:.2e} A_a, d sum A {dA:.2e} A_c, d sum u {du:.2e} '
                  f'(bound {1e-13 * T:.1e})')
            assert dM <= 1e-13 * T and dA <= 1e-13 * T and du <= 1e-13 * T, (name, wname, dM, dA, du)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_a_pairs_sums_depend_only_on_its_rows_and_the_window(dtype):
    """T3, bit for bit: the conn_time power; any pair list; any scale lists; any chunking."""
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ip, ia = pairs_of(C)
    win = (37, 1001)
    la, lb = np.array([4, 0, 3, 2, 2, 0, 1]), np.array([4, 2, 3, 3, 3, 2, 0])      # shuffled, repeated, cross, own
    sph, sam = [3, 1, 1, 5, 0], [5, 8, 4, 4, 1, 6, 7]            # reordered, repeated, 5 and 1 in both lists
    res = {}
    for mb in (C, 2 * C + 3, E * C):
        p = morse_plan(n, dtype, FREQS, mb)
        try:
            res[mb] = p.execute_pac(x, (ip, ia), PHASE, AMP, win)
            assert p.stats()['chunks'] == -(-E // (mb // C))
            if mb == 2 * C + 3:
                lst = p.execute_pac(x, (la, lb), PHASE, AMP, win)
                scl = p.execute_pac(x, (ip, ia), sph, sam, win)
                own = p.execute_pac(x, None, PHASE, AMP, win)
                _, power = p.execute_conn_time(x, ([], []), win, out_kind='cross_sum')
                strided = p.execute_pac(x, (ip, ia), PHASE, AMP, (5, 1021), 4)
                _, spower = p.execute_conn_time(x, ([], []), (5, 1021), 4, out_kind='cross_sum')
        finally:
            p.close()
    M, amp, phase = res[2 * C + 3]
    for mb in (C, E * C):                                         # any chunking
        for u, v in zip(res[mb], res[2 * C + 3]):
            assert np.array_equal(u, v), mb
    # the second amplitude sum is execute_conn_time's power of the same row and window
    assert np.array_equal(amp[..., 1], power[:, :, AMP]) and np.array_equal(strided[1][..., 1], spower[:, :, AMP])
    # indices=None: every channel with itself
    assert own[0].shape == (E, C, len(PHASE), len(AMP)) and np.array_equal(own[0], M[:, :C])
    assert np.array_equal(own[1], amp) and np.array_equal(own[2], phase)
    # any pair list
    assert np.array_equal(lst[1], amp) and np.array_equal(lst[2], phase)
    for k, (a, b) in enumerate(zip(la, lb)):
        q = int(np.flatnonzero((ip == a) & (ia == b))[0])
        assert np.array_equal(lst[0][:, k], M[:, q]), (a, b)
    # any scale lists: a cell is its (phase scale, amplitude scale)'s, wherever it stands
    sM, samp, sphase = scl
    assert sM.shape == (E, len(ip), len(sph), len(sam))
    for i, fp in enumerate(sph):
        for k, fa in enumerate(sam):
            if fp in PHASE and fa in AMP:
                assert np.array_equal(sM[:, :, i, k], M[:, :, PHASE.index(fp), AMP.index(fa)]), (fp, fa)
        if fp in PHASE:
            assert np.array_equal(sphase[:, :, i], phase[:, :, PHASE.index(fp)]), fp
    for k, fa in enumerate(sam):
        if fa in AMP:
            assert np.array_equal(samp[:, :, k], amp[:, :, AMP.index(fa)]), fa
    assert np.array_equal(sM[:, :, 1], sM[:, :, 2]) and np.array_equal(sM[:, :, :, 2], sM[:, :, :, 3])   # the repeats
    assert np.array_equal(samp[:, :, 4, 1], power[:, :, 1])      # scale 1 as an amplitude scale


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_device_tensors_edge_cases_and_errors(dtype):
    """T3: device tensors equal the host call; empty window, E = 0, P = 0; bad arguments raise and the plan
    still works."""
    import torch
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ip, ia = pairs_of(C)
    P, Fp, Fa = len(ip), len(PHASE), len(AMP)
    win = (37, 1001)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        host = p.execute_pac(x, (ip, ia), PHASE, AMP, win)
        tx = torch.from_numpy(np.array(x)).cuda()
        tM = torch.full((E, P, Fp, Fa), float('nan'), dtype=torch.complex128, device='cuda')
        tA = torch.full((E, C, Fa, 2), float('nan'), dtype=torch.float64, device='cuda')
        tU = torch.full((E, C, Fp), float('nan'), dtype=torch.complex128, device='cuda')
        out = p.execute_pac(tx, (ip, ia), PHASE, AMP, win, out=(tM, tA, tU))
        assert out[0] is tM and out[1] is tA and out[2] is tU
        for t, h in zip((tM, tA, tU), host):
            assert np.array_equal(t.cpu().numpy(), h)
        tM2 = torch.full((E, P, Fp, Fa), float('nan'), dtype=torch.complex128, device='cuda')
        p.execute_pac(tx, (ip, ia), PHASE, AMP, win, out=(tM2, None, None))          # no per-channel sums
        assert np.array_equal(tM2.cpu().numpy(), host[0])
        # host output arrays are filled in place; window=None is the whole row
        mine = (np.empty((E, P, Fp, Fa), dtype=np.complex128), None, None)
        got = p.execute_pac(x, (ip, ia), PHASE, AMP, win, out=mine)
        assert got[0] is mine[0] and np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
        full = p.execute_pac(x, (ip, ia), PHASE, AMP)
        for u, v in zip(full, p.execute_pac(x, (ip, ia), PHASE, AMP, (0, n))):
            assert np.array_equal(u, v)
        # an empty window: zero sums; no epochs, no pairs: empty outputs
        for a in p.execute_pac(x, (ip, ia), PHASE, AMP, (n, n)):
            assert not np.any(a) and a.shape[0] == E
        z = p.execute_pac(x[:0], (ip, ia), PHASE, AMP, win)
        assert z[0].shape == (0, P, Fp, Fa) and z[1].shape == (0, C, Fa, 2) and z[2].shape == (0, C, Fp)
        z = p.execute_pac(x, ([], []), PHASE, AMP, win)
        assert z[0].shape == (E, 0, Fp, Fa) and np.array_equal(z[1], host[1]) and np.array_equal(z[2], host[2])
        assert p.stats()['reduce_path'] == L.NW_REDUCE_PAC
        # errors
        for bad in ((-1, 5), (6, 5), (0, n + 1), (0.5, 3), (1,), 7):
            with pytest.raises(ValueError, match='window'):
                p.execute_pac(x, None, PHASE, AMP, bad)
        for step in (0, -1, 1.5):
            with pytest.raises(ValueError, match='step'):
                p.execute_pac(x, None, PHASE, AMP, step=step)
        for bad in ([9], [-1], [], None, [0.5]):
            with pytest.raises(ValueError, match='phase'):
                p.execute_pac(x, None, bad, AMP)
            with pytest.raises(ValueError, match='amp'):
                p.execute_pac(x, None, PHASE, bad)
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_pac(x, (ip, ia), PHASE, AMP, out=(np.empty((E, P, Fp, Fa)), None, None))
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_pac(x, (ip, ia), PHASE, AMP, out=(None, np.empty((E, C, Fa)), None))
        with pytest.raises(ValueError, match='indices'):
            p.execute_pac(x, ([0], [C]), PHASE, AMP)
        with pytest.raises(ValueError, match='epochs, channels'):
            p.execute_pac(x.reshape(E * C, n), None, PHASE, AMP)
        with pytest.raises(ValueError, match='output'):
            p.execute_pac(tx, (ip, ia), PHASE, AMP)
        with pytest.raises(ValueError, match='complex128'):
            p.execute_pac(tx, (ip, ia), PHASE, AMP, out=(tA, tA, tU))
        with pytest.raises(ValueError, match='hold'):
            p.execute_pac(tx, (ip, ia), PHASE, AMP, out=(tM[:2], tA, tU))
        # the C ABI's own checks: a scale position outside the plan's list
        import ctypes
        V_ = ctypes.c_void_p
        xc = np.ascontiguousarray(x)
        ii = ip.astype(np.int32)
        badf, okf = np.array([0, 9], dtype=np.int32), np.array([4, 5], dtype=np.int32)
        buf = np.empty((E, P, 2, 2), dtype=np.complex128)
        for fa_, fb_, word in ((badf, okf, b'phase scale 1 = 9'), (okf, badf, b'amplitude scale 1 = 9')):
            rc = L.lib().nw_execute_pac(p.handle, xc.ctypes.data_as(V_), E, C, ii.ctypes.data_as(V_), ii.ctypes.data_as(V_),
                                        len(ii), fa_.ctypes.data_as(V_), 2, fb_.ctypes.data_as(V_), 2, 0, n, 1,
                                        buf.ctypes.data_as(V_), None, None, L.NW_MEM_HOST)
            assert rc == L.NW_E_INVALID and word in L.lib().nw_last_error(), L.lib().nw_last_error()
        small = morse_plan(n, dtype, FREQS, C - 1)
        try:
            with pytest.raises(ValueError, match='max_batch'):
                small.execute_pac(x, None, PHASE, AMP)
        finally:
            small.close()
        again = p.execute_pac(x, (ip, ia), PHASE, AMP, win)                           # the plan still works
        for u, v in zip(again, host):
            assert np.array_equal(u, v)
        # ... and the over-time call on the same plan is what it was
        assert p.execute_conn_time(x, out_kind='lag_sum').shape == (E, C * (C - 1) // 2, len(FREQS), 4)
        assert p.stats()['reduce_path'] == L.NW_REDUCE_CONN_TIME
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
    ip, ia = pairs_of(C)
    tol = tol_of(n, dtype)
    idx = np.arange(*win)
    T = len(idx)
    Ac = np.max(np.abs(y), axis=(2, 3))
    rM, ramp, rphase, A, mp = ref_sums(y, ip, ia, PHASE, AMP, idx)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        M, amp, phase = p.execute_pac(x, (ip, ia), PHASE, AMP, win)
    finally:
        p.close()
    if dtype == 'float64':
        for kind in KINDS:
            dv = np.abs(finalize_pac(kind, M, amp, phase, ip, ia, T) - finalize_pac(kind, rM, ramp, rphase, ip, ia, T)).max()
            print(f'n={n} {win} fp64 {kind}: {dv:.2e}')
            assert dv <= 1e-7, (kind, dv)
        return
    bM, _ = t1_bounds(A, mp, Ac, ip, ia, tol)
    Aa = Ac[:, ia][:, :, None, None]
    den = np.sqrt(T * ramp[:, ia][:, :, None, :, 1]) - 2 * tol * T * Aa
    assert np.all(den > 0), den.min()                             # on the reference alone
    bound = (bM + 2 * tol * T * Aa) / den
    d = np.abs(finalize_pac('direct_pac', M, amp, phase, ip, ia, T) - finalize_pac('direct_pac', rM, ramp, rphase, ip, ia, T))
    print(f'n={n} {win} fp32: direct_pac worst {np.max(d / bound):.3f} of its bound (largest bound {bound.max():.2e})')
    assert np.all(d <= bound), np.max(d / bound)


def test_class_layer():
    """T5: pac_batch is finalize_pac of Plan.execute_pac, with device decim and with host decim; average;
    cross-channel indices; EpochsWavelet.pac's concatenated scale list and padding."""
    E, C = 3, 5
    own = np.arange(C)
    cross = (np.array([0, 2, 1]), np.array([2, 1, 1]))
    # device decim: n = 4096, decim 4, window in full-rate samples
    n, dtype = 4096, 'float32'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype)
    win = (150, 4001)
    t0, t1, step, T = time_window(n, 4, win, True)
    assert (t0, t1, step, T) == (38, 1001, 1, 963)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, decim=4)
    try:
        sums = p.execute_pac(x, None, PHASE, AMP, (t0, t1), step)
        csums = p.execute_pac(x, cross, PHASE, AMP, (t0, t1), step)
    finally:
        p.close()
    for out in KINDS:
        want = finalize_pac(out, *sums, own, own, T)
        got = w.pac_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, window=win, decim=4)
        assert got.shape == (E, C, len(PHASE), len(AMP)) and np.array_equal(got, want, equal_nan=True), out
        avg = w.pac_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, window=win, decim=4, average=True)
        assert avg.shape == (C, len(PHASE), len(AMP)) and np.array_equal(avg, want.mean(axis=0), equal_nan=True), out
        got = w.pac_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, indices=cross, window=win, decim=4)
        assert np.array_equal(got, finalize_pac(out, *csums, *cross, T), equal_nan=True), out
    got = w.pac_batch(x, FREQS, phase=PHASE, amp=AMP, out='pac_sum', window=win, decim=4)
    for u, v in zip(got, sums):
        assert np.array_equal(u, v)
    assert w.pac_batch(x, FREQS, phase=PHASE, amp=AMP).shape == (E, C, len(PHASE), len(AMP))     # direct_pac
    st = w.plan_stats()[-1]                                        # the most recent plan: the full-rate one
    assert st['reduce_path'] == L.NW_REDUCE_PAC
    # host decim: the rocFFT engine has no device decimation: a full-rate plan, step = decim
    n, dtype = 1000, 'float64'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype, engine='rocfft')
    win = (37, 990)
    t0, t1, step, T = time_window(n, 4, win, False)
    assert (t0, t1, step, T) == (40, 990, 4, 238)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, engine='rocfft')
    try:
        sums = p.execute_pac(x, cross, PHASE, AMP, (t0, t1), step)
    finally:
        p.close()
    for out in KINDS:
        got = w.pac_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, indices=cross, window=win, decim=4)
        assert np.array_equal(got, finalize_pac(out, *sums, *cross, T)), out
    # EpochsWavelet: the two frequency lists concatenated, padding in seconds, channels picked by name
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)                 # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype, engine='rocfft'))
    sub = np.ascontiguousarray(x[:, :3])
    pf, af = [FREQS[i] for i in PHASE], [FREQS[i] for i in AMP]
    idx = ([2, 0], [0, 1])
    for method in KINDS:
        assert np.array_equal(ew.pac(['a', 'b', 'c'], pf, af, method=method, padding=0.0371),
                              w.pac_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, window=(37, n - 37))), method
        assert np.array_equal(ew.pac(['a', 'b', 'c'], pf, af, method=method, indices=idx, padding=0.1, decim=4, average=True),
                              w.pac_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, indices=idx, window=(100, 900),
                                          decim=4, average=True)), method
    assert np.array_equal(ew.pac(['a', 'b', 'c'], pf, af), w.pac_batch(sub, FREQS, phase=PHASE, amp=AMP))
    with pytest.raises(ValueError, match='padding'):
        ew.pac(['a', 'b'], pf, af, padding=0.5)


def test_pac_under_bounds_checks():
    """T6: the debug library (kernel bounds checks, nw_dcheck.h) on n = 1024, on a tail tile (n = 1201) and on
    partial scale tiles (9 x 17 scales), five windows, own and cross-channel pairs: no check fails."""
    body = ('rng = np.random.default_rng(1)\n'
            'for tag, n, E, C, dt, F, ph, am in (("a", 1024, 3, 5, "float32", 9, [0, 1, 2, 3], [4, 5, 6, 7, 8]),\n'
            '                                    ("b", 1201, 3, 5, "float64", 3, [0], [1, 2]),\n'
            '                                    ("c", 1024, 2, 2, "float64", 26, list(range(9)), list(range(9, 26)))):\n'
            '    x = rng.standard_normal((E, C, n)).astype(dt)\n'
            '    p = nw.Plan(n, F, dt, max_batch=2 * C + 3)\n'
            '    p.set_wavelet("morse", [17.5, 3.], np.geomspace(3., 300., F), L.trans_grid(n / 1000., 1000., False))\n'
            '    ok = True\n'
            '    for win, step in ((None, 1), ((37, 1001), 1), ((0, 1), 1), ((5, n), 4), ((9, 9), 1)):\n'
            '        own = p.execute_pac(x, None, ph, am, win, step)\n'
            '        short = p.execute_pac(x, ([C - 1, 0, 1], [0, 0, 1]), am[:1] + ph, ph[:1] + am, win, step)\n'
            '        for a in own + short:\n'
            '            ok = ok and bool(np.all(np.isfinite(a))) and a.shape[0] == E\n'
            '    print("ok", tag, ok)\n'
            '    p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok a True' in lines and 'ok b True' in lines and 'ok c True' in lines, lines
