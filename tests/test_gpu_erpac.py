"""GPU tests of event-related phase-amplitude coupling: nw_execute_erpac (nw_erpac_kernel and nw_erpac_rows_kernel,
nw_erpac.hip) through Plan.execute_erpac, engine.finalize_erpac, WaveletBase.erpac_batch and EpochsWavelet.erpac.

For a pair (p, a) of a phase and an amplitude channel with rows y_e,c (F, n_out) of epoch e, listed phase scales
fph, amplitude scales fam and a window of T samples s_j = t0 + j step, with A = |y_a[fa, s_j]| and
u = c + i s = y_p[fp, s_j] / |y_p[fp, s_j]|, the sums run over the epochs e at every sample:
    M = sum_e A u (P, Fp, Fa, T),  amp = {sum_e A, sum_e A^2} (C, Fa, T, 2),
    phase = the planes sum_e c, s, c^2, s^2, c s (C, Fp, 5, T).
References are formed here from oracle.nw_oracle in complex128.

Inputs: the coupled recipe of epoch_cases.py (a 70 Hz amplitude that follows the 7 Hz phase on every even channel,
the phase drawn per epoch), sfreq 1000, Morse(1000) with its default b, r, FREQS (nine scales), phase = [0, 1, 2, 3],
amp = [4 .. 8].  PAIRS are test_gpu_pac.py's: every channel with itself, then three cross-channel pairs.  The sum
tests take E = 5, C = 5, max_batch = 2 C + 3 (chunks of 2, 2 and 1 epochs); the measure tests E = 24, C = 3,
max_batch = 7 C (chunks of 7, 7, 7 and 3 epochs).  Forms: the epoch-axis rows of epoch_cases.py but the 17-channel one
(pairs are not tiled here), the two-pass row on (2, 3, FREQS3), and one row of 26 scales with 9 phase and 17 amplitude
positions (partial tiles on both scale axes).  Windows (the plan's output samples): full, (0, 1), (37, 1001), an empty
one and a stride-4 one (at n = 1201 the last sample tile has 49 live lanes); the full-rate n = 1000 plan of the rocFFT
form takes them through engine.time_window with decim = 4 (its step-4 path).

tol = tol_of(n, dtype): 1e-12 fp64, 1e-5 fp32, 2e-5 fp32 on chirp-z lengths; A_{e,c}: max |y| over (F, N) of the oracle's
undecimated rows of epoch e, channel c; u_e = min(2, 2 tol A_{e,p} / |y_p|) at the sample (a unit phasor moves by at
most 2 |dy| / |y|).
  T1  against the oracle, per output value: |dM| <= sum_e [2 tol A_{e,a} (1 + u_e) + |y_a| u_e] + 1e-13 sum_e A_{e,a};
      |d sum A| <= 2 tol sum_e A_{e,c}; |d sum A^2| <= 4 tol sum_e A_{e,c}^2; |d sum c|, |d sum s| <= sum_e u_e + 1e-13 E;
      |d sum c^2|, |d sum s^2|, |d sum c s| <= sum_e (2 + u_e) u_e + 1e-13 E (test_gpu_pac.py's T1 terms with e for j; a
      product of two components of unit phasors moves by at most (2 + u) u).
  T2  fp64: the same plan's own rows reduced in numpy in epoch order: sum (re^2 + im^2) array_equal; every other sum
      within 1e-13 sum_e (A_{e,a}, A_{e,c}, 1) (hypot and the division may differ in the last place).
  T3  bit for bit, fp32 and fp64: amp[..., 1] is execute_conn's power; a pair's M under any pair list, any phase /
      amp lists, any max_batch, host arrays and device tensors; every windowed result is the matching slice of the
      full-window result.
  T4  measures: fp64 every kind within 1e-7 of the formula on the oracle's sums; fp32 direct_pac: test_gpu_pac.py's
      bound with E for T; fp32 circular: |d rho| <= 2 b on every cell with b <= 0.05, b the first-order propagation
      of the T1 bounds through rho (central differences at the oracle's sums), the factor 2 for the second order.
  T5  the layers; T6 the debug library."""
import os

import numpy as np
import pytest

from epoch_cases import (EPOCH_AXIS, FREQS, SHAPES, FakeEpochs, coupled_rows, forms, morse_plan, run_under_bounds_checks,
                         tol_of, windows_of)

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import finalize_erpac, time_window  # noqa: E402

PHASE, AMP = [0, 1, 2, 3], [4, 5, 6, 7, 8]
FREQS26 = [float(f) for f in np.round(np.geomspace(4., 300., 26), 2)]
SHARED = ('mvl', 'mvl_norm', 'direct_pac', 'debiased_pac')
KINDS = ('circular', 'circular_pval') + SHARED
# (phase channel, amplitude channel): every channel with itself, then three cross-channel pairs (test_gpu_pac.py's)
PAIRS = (np.array([0, 1, 2, 3, 4, 0, 1, 2]), np.array([0, 1, 2, 3, 4, 2, 0, 3]))


def pairs_of(C):
    ip, ia = PAIRS
    keep = (ip < C) & (ia < C)
    return ip[keep], ia[keep]


def ref_sums(y, ip, ia, fph, fam, idx):
    """The oracle's sums over the epochs at the samples ``idx`` of rows y (E, C, F, n): (M, amp, phase, |y_amp|
    (E, C, Fa, T), |y_phase| (E, C, Fp, T))."""
    yw = y[..., idx]
    ya, yp = yw[:, :, fam], yw[:, :, fph]
    A, mp = np.abs(ya), np.abs(yp)
    with np.errstate(invalid='ignore', divide='ignore'):
        u = yp / mp
    c, s = u.real, u.imag
    M = np.einsum('epit,epkt->pikt', u[:, ip], A[:, ia].astype(np.complex128))
    amp = np.stack([A.sum(0), (ya.real ** 2 + ya.imag ** 2).sum(0)], axis=-1)
    phase = np.stack([c.sum(0), s.sum(0), (c * c).sum(0), (s * s).sum(0), (c * s).sum(0)], axis=2)
    return M, amp, phase, A, mp


def t1_bounds(A, mp, Ac, ip, ia, tol):
    """The T1 bounds: (bM (P, Fp, Fa, T), bA (C), bA2 (C), bu (C, Fp, T), bu2 (C, Fp, T)); bu and bu2 without their
    1e-13 E."""
    with np.errstate(divide='ignore'):
        u = np.minimum(2., 2 * tol * Ac[:, :, None, None] / mp)                  # (E, C, Fp, T)
    bu, bu2 = u.sum(0), ((2. + u) * u).sum(0)
    sAc = Ac.sum(0)
    bM = (2 * tol * (sAc[ia][:, None, None, None] + np.einsum('ep,epit->pit', Ac[:, ia], u[:, ip])[:, :, None])
          + np.einsum('epkt,epit->pikt', A[:, ia], u[:, ip]) + 1e-13 * sAc[ia][:, None, None, None])
    return bM, 2 * tol * sAc, 4 * tol * (Ac ** 2).sum(0), bu, bu2


def check_t1(name, got, y, Ac, ip, ia, fph, fam, idx, tol):
    """T1 of (M, amp, phase) at the window samples ``idx`` (indices into the reference rows)."""
    M, amp, phase = got
    E = y.shape[0]
    rM, ramp, rphase, A, mp = ref_sums(y, ip, ia, fph, fam, idx)
    assert M.shape == rM.shape and amp.shape == ramp.shape and phase.shape == rphase.shape, name
    bM, bA, bA2, bu, bu2 = t1_bounds(A, mp, Ac, ip, ia, tol)
    dM = np.abs(M - rM)
    dA = np.abs(amp[..., 0] - ramp[..., 0]) / bA[:, None, None]
    dA2 = np.abs(amp[..., 1] - ramp[..., 1]) / bA2[:, None, None]
    du = np.abs(phase - rphase)
    over1 = np.max(du[:, :, :2] - bu[:, :, None] - 1e-13 * E)
    over2 = np.max(du[:, :, 2:] - bu2[:, :, None] - 1e-13 * E)
    print(f'{name} T1: dM {np.max(dM / bM):.3f}, d sum A {dA.max():.3f}, d sum A^2 {dA2.max():.3f} of their bounds '
          f'(tol {tol:.0e}); d sum c, s {over1:.3e}, d sum c^2, s^2, cs {over2:.3e} over their bounds')
    assert np.all(dM <= bM), (name, np.max(dM / bM))
    assert dA.max() <= 1 and dA2.max() <= 1, (name, dA.max(), dA2.max())
    assert over1 <= 0 and over2 <= 0, (name, over1, over2)


def own_sums(rows, ip, ia, fph, fam, idx):
    """(M, amp, phase) of the plan's own complex128 rows (E, C, F, n_out), every value added in epoch order from 0."""
    yw = rows[..., idx]
    re, im = np.ascontiguousarray(yw.real), np.ascontiguousarray(yw.imag)
    E, C = rows.shape[:2]
    T = len(idx)
    M = np.zeros((len(ip), len(fph), len(fam), T), dtype=np.complex128)
    amp = np.zeros((C, len(fam), T, 2))
    phase = np.zeros((C, len(fph), 5, T))
    for e in range(E):
        ar, ai = re[e][:, fam], im[e][:, fam]
        A = np.hypot(ar, ai)                                                       # (C, Fa, T)
        amp[..., 0] = amp[..., 0] + A
        amp[..., 1] = amp[..., 1] + (ar * ar + ai * ai)
        with np.errstate(invalid='ignore', divide='ignore'):
            h = np.hypot(re[e][:, fph], im[e][:, fph])
            c, s = re[e][:, fph] / h, im[e][:, fph] / h                            # (C, Fp, T)
        for k, term in enumerate((c, s, c * c, s * s, c * s)):
            phase[:, :, k] = phase[:, :, k] + term
        Aa = A[ia][:, None]                                                        # (P, 1, Fa, T)
        M.real = M.real + Aa * c[ip][:, :, None]
        M.imag = M.imag + Aa * s[ip][:, :, None]
    return M, amp, phase


# (id, n, dtype, E, C, freqs, phase, amp, plan keywords, device decim, host decim, kernel of the form)
CASES = []
for name, n, dtype, kw, decim, host_decim, kernel in forms(*[i for i in EPOCH_AXIS if i != 'tiles-17ch-f64']):
    E, C, freqs = SHAPES.get(name, (5, 5, FREQS))
    fph, fam = (PHASE, AMP) if freqs is FREQS else ([0], [1, 2])
    # the rocFFT engine has no device decimation: its windows are those of a full-rate plan at decim = 4
    CASES.append((name, n, dtype, E, C, freqs, fph, fam, kw, decim, 4 if kw.get('engine') == 'rocfft' else host_decim,
                  kernel))
# 9 phase x 17 amplitude positions: two phase tiles and two amplitude tiles, one of each partial
CASES.append(('tiles-9x17-f64', 1024, 'float64', 5, 2, FREQS26, list(range(9)), list(range(9, 26)), {}, 1, 1,
              'nw_fused_kernel'))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 for every case and window, T2 for the fp64 cases, T3's windows; PAIRS; max_batch = 2 C + 3."""
    name, n, dtype, E, C, freqs, fph, fam, kw, decim, host_decim, kernel = case
    x, y = coupled_rows(n, E, C, dtype, freqs)
    Ac = np.max(np.abs(y), axis=(2, 3))                       # (E, C), of the undecimated rows
    ip, ia = pairs_of(C)
    tol = tol_of(n, dtype)
    n_out = n // decim
    p = morse_plan(n, dtype, freqs, 2 * C + 3, decim=decim, **kw)
    try:
        assert p.n_out == n_out
        got = {}
        for wname, win, step in windows_of(n, n_out, host_decim) + [('every', (0, n_out), 1)]:
            got[wname] = (win, step, p.execute_erpac(x, (ip, ia), fph, fam, win, step))
            st = p.stats()
            assert st['reduce_path'] == L.NW_REDUCE_ERPAC and L.KERNEL_NAMES[st['kernel']] == kernel, (name, st)
        assert st['chunks'] == len(got) * -(-E // ((2 * C + 3) // C)), (name, st)
        rows = None
        if dtype == 'float64':
            rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, len(freqs), n_out)
    finally:
        p.close()
    every = got.pop('every')[2]                                # every output sample: what a window is a slice of
    for wname, (win, step, sums) in got.items():
        idx = np.arange(win[0], win[1], step)
        T = len(idx)
        assert T == L.conn_time_count(n_out, win[0], win[1], step)
        M, amp, phase = sums
        assert M.dtype == np.complex128 and amp.dtype == np.float64 and phase.dtype == np.float64
        assert M.shape == (len(ip), len(fph), len(fam), T) and amp.shape == (C, len(fam), T, 2)
        assert phase.shape == (C, len(fph), 5, T)
        # T3: a value depends on its rows and its sample, not on the window
        assert np.array_equal(M, every[0][..., idx]) and np.array_equal(amp, every[1][:, :, idx]), (name, wname)
        assert np.array_equal(phase, every[2][..., idx]), (name, wname)
        if T == 0:
            continue
        check_t1(f'{name} {wname}', sums, y, Ac, ip, ia, fph, fam, idx * decim, tol)
        if rows is not None:                                   # T2
            oM, oamp, ophase = own_sums(rows, ip, ia, fph, fam, idx)
            assert np.array_equal(amp[..., 1], oamp[..., 1]), (name, wname, np.abs(amp - oamp)[..., 1].max())
            sAc = Ac.sum(0)
            dM = np.max(np.abs(M - oM) / sAc[ia][:, None, None, None])
            dA = np.max(np.abs(amp[..., 0] - oamp[..., 0]) / sAc[:, None, None])
            du = np.abs(phase - ophase).max()
            print(f'{name} {wname} T2: sum A^2 equal bit for bit; dM {dM:.2e} sum A_a, d sum A {dA:.2e} sum A_c, d phase '
                  f'sums {du:.2e} (bound {1e-13 * E:.1e})')
            assert dM <= 1e-13 and dA <= 1e-13 and du <= 1e-13 * E, (name, wname, dM, dA, du)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_a_value_depends_only_on_its_rows_and_its_sample(dtype):
    """T3, bit for bit: execute_conn's power; any pair list; any scale lists; any chunking; device tensors; the
    empty cases and the errors."""
    import torch
    n, E, C = 1024, 5, 5
    x, _ = coupled_rows(n, E, C, dtype, FREQS)
    ip, ia = pairs_of(C)
    P, Fp, Fa = len(ip), len(PHASE), len(AMP)
    win = (37, 1001)
    T = win[1] - win[0]
    la, lb = np.array([4, 0, 3, 2, 2, 0, 1]), np.array([4, 2, 3, 3, 3, 2, 0])      # shuffled, repeated, cross, own
    sph, sam = [3, 1, 1, 5, 0], [5, 8, 4, 4, 1, 6, 7]            # reordered, repeated, 5 and 1 in both lists
    res = {}
    for mb in (C, 2 * C + 3, E * C):                              # one epoch per chunk; 2, 2, 1; all in one chunk
        p = morse_plan(n, dtype, FREQS, mb)
        try:
            res[mb] = p.execute_erpac(x, (ip, ia), PHASE, AMP, win)
            assert p.stats()['chunks'] == -(-E // (mb // C))
            if mb == 2 * C + 3:
                lst = p.execute_erpac(x, (la, lb), PHASE, AMP, win)
                scl = p.execute_erpac(x, (ip, ia), sph, sam, win)
                own = p.execute_erpac(x, None, PHASE, AMP, win)
                _, power = p.execute_conn(x, ([], []), out_kind='cross_sum')
                # device tensors
                tx = torch.from_numpy(np.array(x)).cuda()
                tM = torch.full((P, Fp, Fa, T), float('nan'), dtype=torch.complex128, device='cuda')
                tA = torch.full((C, Fa, T, 2), float('nan'), dtype=torch.float64, device='cuda')
                tU = torch.full((C, Fp, 5, T), float('nan'), dtype=torch.float64, device='cuda')
                out = p.execute_erpac(tx, (ip, ia), PHASE, AMP, win, out=(tM, tA, tU))
                assert out[0] is tM and out[1] is tA and out[2] is tU
                dev = [t.cpu().numpy() for t in (tM, tA, tU)]
                tM2 = torch.full((P, Fp, Fa, T), float('nan'), dtype=torch.complex128, device='cuda')
                p.execute_erpac(tx, (ip, ia), PHASE, AMP, win, out=(tM2, None, None))    # no per-channel sums
                dev2 = tM2.cpu().numpy()
                # host output arrays are filled in place
                mine = (np.empty((P, Fp, Fa, T), dtype=np.complex128), None, None)
                inplace = p.execute_erpac(x, (ip, ia), PHASE, AMP, win, out=mine)
                assert inplace[0] is mine[0]
                # the empty cases: no samples, no epochs (zero sums), no pairs
                z = p.execute_erpac(x, (ip, ia), PHASE, AMP, (n, n))
                assert z[0].shape == (P, Fp, Fa, 0) and z[1].shape == (C, Fa, 0, 2) and z[2].shape == (C, Fp, 5, 0)
                z = p.execute_erpac(x[:0], (ip, ia), PHASE, AMP, win)
                assert z[0].shape == (P, Fp, Fa, T) and not np.any(z[0]) and not np.any(z[1]) and not np.any(z[2])
                nopair = p.execute_erpac(x, ([], []), PHASE, AMP, win)
                assert p.stats()['reduce_path'] == L.NW_REDUCE_ERPAC
                # errors: the plan still works afterwards
                for bad in ((-1, 5), (6, 5), (0, n + 1), (0.5, 3), (1,), 7):
                    with pytest.raises(ValueError, match='window'):
                        p.execute_erpac(x, None, PHASE, AMP, bad)
                with pytest.raises(ValueError, match='step'):
                    p.execute_erpac(x, None, PHASE, AMP, step=0)
                for bad in ([9], [-1], [], None, [0.5]):
                    with pytest.raises(ValueError, match='phase'):
                        p.execute_erpac(x, None, bad, AMP)
                    with pytest.raises(ValueError, match='amp'):
                        p.execute_erpac(x, None, PHASE, bad)
                with pytest.raises(ValueError, match='right dtype and size'):
                    p.execute_erpac(x, (ip, ia), PHASE, AMP, win, out=(np.empty((P, Fp, Fa, T)), None, None))
                with pytest.raises(ValueError, match='indices'):
                    p.execute_erpac(x, ([0], [C]), PHASE, AMP)
                with pytest.raises(ValueError, match='output'):
                    p.execute_erpac(tx, (ip, ia), PHASE, AMP)
                with pytest.raises(ValueError, match='complex128'):
                    p.execute_erpac(tx, (ip, ia), PHASE, AMP, win, out=(tA, tA, tU))
                with pytest.raises(ValueError, match='hold'):
                    p.execute_erpac(tx, (ip, ia), PHASE, AMP, win, out=(tM[:2], tA, tU))
                import ctypes
                V_ = ctypes.c_void_p
                xc, ii = np.ascontiguousarray(x), ip.astype(np.int32)
                badf, okf = np.array([0, 9], dtype=np.int32), np.array([4, 5], dtype=np.int32)
                buf = np.empty((P, 2, 2, T), dtype=np.complex128)
                for fa_, fb_, word in ((badf, okf, b'phase scale 1 = 9'), (okf, badf, b'amplitude scale 1 = 9')):
                    rc = L.lib().nw_execute_erpac(p.handle, xc.ctypes.data_as(V_), E, C, ii.ctypes.data_as(V_),
                                                  ii.ctypes.data_as(V_), len(ii), fa_.ctypes.data_as(V_), 2,
                                                  fb_.ctypes.data_as(V_), 2, win[0], win[1], 1, buf.ctypes.data_as(V_), None,
                                                  None, L.NW_MEM_HOST)
                    assert rc == L.NW_E_INVALID and word in L.lib().nw_last_error(), L.lib().nw_last_error()
                again = p.execute_erpac(x, (ip, ia), PHASE, AMP, win)
        finally:
            p.close()
    small = morse_plan(n, dtype, FREQS, C - 1)
    try:
        with pytest.raises(ValueError, match='max_batch'):
            small.execute_erpac(x, None, PHASE, AMP)
    finally:
        small.close()
    M, amp, phase = res[2 * C + 3]
    for mb in (C, E * C):                                         # any chunking
        for u, v in zip(res[mb], res[2 * C + 3]):
            assert np.array_equal(u, v), mb
    for u, v in zip(again, res[2 * C + 3]):
        assert np.array_equal(u, v)
    # device tensors and host arrays
    for u, v in zip(dev, res[2 * C + 3]):
        assert np.array_equal(u, v)
    assert np.array_equal(dev2, M) and np.array_equal(inplace[0], M) and np.array_equal(inplace[1], amp)
    # the second amplitude sum is execute_conn's power of the same rows and samples
    assert np.array_equal(amp[..., 1], power[:, AMP, win[0]:win[1]])
    # no pairs: the per-channel sums alone
    assert nopair[0].shape == (0, Fp, Fa, T) and np.array_equal(nopair[1], amp) and np.array_equal(nopair[2], phase)
    # indices=None: every channel with itself
    assert own[0].shape == (C, Fp, Fa, T) and np.array_equal(own[0], M[:C])
    assert np.array_equal(own[1], amp) and np.array_equal(own[2], phase)
    # any pair list
    assert np.array_equal(lst[1], amp) and np.array_equal(lst[2], phase)
    for k, (a, b) in enumerate(zip(la, lb)):
        q = int(np.flatnonzero((ip == a) & (ia == b))[0])
        assert np.array_equal(lst[0][k], M[q]), (a, b)
    # any scale lists: a cell is its (phase scale, amplitude scale)'s, wherever it stands
    sM, samp, sphase = scl
    assert sM.shape == (P, len(sph), len(sam), T)
    for i, fp in enumerate(sph):
        for k, fa in enumerate(sam):
            if fp in PHASE and fa in AMP:
                assert np.array_equal(sM[:, i, k], M[:, PHASE.index(fp), AMP.index(fa)]), (fp, fa)
        if fp in PHASE:
            assert np.array_equal(sphase[:, i], phase[:, PHASE.index(fp)]), fp
    for k, fa in enumerate(sam):
        if fa in AMP:
            assert np.array_equal(samp[:, k], amp[:, AMP.index(fa)]), fa
    assert np.array_equal(sM[:, 1], sM[:, 2]) and np.array_equal(sM[:, :, 2], sM[:, :, 3])       # the repeats
    assert np.array_equal(samp[:, 4, :, 1], power[:, 1, win[0]:win[1]])      # scale 1 as an amplitude scale


def rho_of(mr, mi, sa, saa, sc, ss, scc, sss, scs, E):
    """The circular-linear correlation from the nine sums (this file's own restatement, no zero conventions)."""
    def r(sxy, sx, sy, sxx, syy):
        return (sxy - sx * sy / E) / np.sqrt((sxx - sx * sx / E) * (syy - sy * sy / E))
    rxc, rxs, rcs = r(mr, sa, sc, saa, scc), r(mi, sa, ss, saa, sss), r(scs, sc, ss, scc, sss)
    return np.sqrt(np.maximum((rxc * rxc + rxs * rxs - 2 * rxc * rxs * rcs) / (1 - rcs * rcs), 0.))


def rho_bound(rM, ramp, rphase, bounds, Ac, E):
    """b (C, Fp, Fa, T): the T1 bounds propagated to first order through rho for own-channel pairs, the nine
    derivatives by central differences at the oracle's sums (steps of 1e-6 of each sum's scale)."""
    bM, bA, bA2, bu, bu2 = bounds
    sAc, sAc2 = Ac.sum(0), (Ac ** 2).sum(0)
    q = [rM.real, rM.imag, ramp[:, None, :, :, 0], ramp[:, None, :, :, 1]] + [rphase[:, :, None, k] for k in range(5)]
    scale = [sAc[:, None, None, None]] * 3 + [sAc2[:, None, None, None]] + [float(E)] * 5
    bq = [bM, bM, bA[:, None, None, None], bA2[:, None, None, None]] + [bu[:, :, None] + 1e-13 * E] * 2 + \
        [bu2[:, :, None] + 1e-13 * E] * 3
    b = np.zeros(rM.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        for k in range(9):
            h = 1e-6 * scale[k]
            up, dn = list(q), list(q)
            up[k], dn[k] = q[k] + h, q[k] - h
            b = b + np.abs(rho_of(*up, E) - rho_of(*dn, E)) / (2 * h) * bq[k]
    return np.where(np.isfinite(b), b, np.inf)


def check_planted(name, rho, pval, rphase, E):
    """On the oracle alone: the conditions of the planted coupling (printed)."""
    sc, ss, scc, sss, scs = (rphase[:, :, k] for k in range(5))
    vc, vs = scc - sc * sc / E, sss - ss * ss / E
    rcs = (scs - sc * ss / E) / np.sqrt(vc * vs)
    cell = (slice(None), PHASE.index(1), AMP.index(5))             # (7 Hz, 70 Hz)
    sig = np.mean(pval[1] < 0.01)
    print(f'{name}: reference: 1 - r_cs^2 >= {np.min(1 - rcs * rcs):.3f}, var(c) / E >= {np.min(vc / E):.3f}; planted cell of '
          f'channels 0 and 2: rho >= {min(rho[0][cell[1:]].min(), rho[2][cell[1:]].min()):.3f}, p <= '
          f'{max(pval[0][cell[1:]].max(), pval[2][cell[1:]].max()):.2e}; channel 1: median rho {np.median(rho[1]):.3f}, '
          f'p < 0.01 on {100 * sig:.2f} % of cells and samples')
    assert np.min(1 - rcs * rcs) >= 0.5 and np.min(vc / E) >= 0.1, name
    for ch in (0, 2):
        assert rho[ch][cell[1:]].min() >= 0.8 and pval[ch][cell[1:]].max() < 0.01, (name, ch)
    assert np.median(rho[1]) <= 0.3 and sig <= 0.02, (name, np.median(rho[1]), sig)


T4_WINDOWS = {'full': lambda n: ((0, n), 1), 'inner': lambda n: ((37, 1001), 1), 'stride': lambda n: ((5, n - 3), 4)}
T4_CASES = [(n, dtype, w) for dtype in ('float32', 'float64') for n in (1024, 1201) for w in T4_WINDOWS]


@pytest.mark.parametrize('case', T4_CASES, ids=[f'{n}-{d}-{w}' for n, d, w in T4_CASES])
def test_measures(case):
    """T4: E = 24, C = 3, own-channel pairs, max_batch = 7 C (chunks of 7, 7, 7 and 3 epochs)."""
    n, dtype, wname = case
    E, C = 24, 3
    win, step = T4_WINDOWS[wname](n)
    x, y = coupled_rows(n, E, C, dtype, FREQS)
    own = np.arange(C)
    tol = tol_of(n, dtype)
    idx = np.arange(win[0], win[1], step)
    Ac = np.max(np.abs(y), axis=(2, 3))
    rM, ramp, rphase, A, mp = ref_sums(y, own, own, PHASE, AMP, idx)
    ref = {kind: finalize_erpac(kind, rM, ramp, rphase, own, own, E) for kind in KINDS}
    check_planted(f'n={n} {dtype} {wname}', ref['circular'], ref['circular_pval'], rphase, E)
    bounds = t1_bounds(A, mp, Ac, own, own, tol)
    b = rho_bound(rM, ramp, rphase, bounds, Ac, E)
    p = morse_plan(n, dtype, FREQS, 7 * C)
    try:
        M, amp, phase = p.execute_erpac(x, None, PHASE, AMP, win, step)
        assert p.stats()['chunks'] == 4
    finally:
        p.close()
    got = {kind: finalize_erpac(kind, M, amp, phase, own, own, E) for kind in KINDS}
    if dtype == 'float64':
        print(f'n={n} {wname} fp64: the propagated bound of rho on the oracle <= {b.max():.2e}')
        assert b.max() <= 1e-7, b.max()                            # on the reference alone: the tolerance covers it
        for kind in KINDS:
            dv = np.abs(got[kind] - ref[kind]).max()
            print(f'n={n} {wname} fp64 {kind}: {dv:.2e}')
            assert dv <= 1e-7, (kind, dv)
        return
    # fp32 direct_pac: test_gpu_pac.py's T4 bound with the epochs in the place of the samples
    sAa = Ac.sum(0)[:, None, None, None]
    den = np.sqrt(E * ramp[:, None, :, :, 1]) - 2 * tol * sAa
    assert np.all(den > 0), den.min()                              # on the reference alone
    bound = (bounds[0] + 2 * tol * sAa) / den
    d = np.abs(got['direct_pac'] - ref['direct_pac'])
    print(f'n={n} {wname} fp32: direct_pac worst {np.max(d / bound):.3f} of its bound (largest bound {bound.max():.2e})')
    assert np.all(d <= bound), np.max(d / bound)
    # fp32 circular: on every cell whose propagated bound is at most 0.05; at most 1 % of the cells are left out
    keep = b <= 0.05
    left = 1 - np.mean(keep)
    d = np.abs(got['circular'] - ref['circular'])
    print(f'n={n} {wname} fp32: circular: {100 * left:.2f} % of the cells left out (b > 0.05); worst '
          f'{np.max(d[keep] / (2 * b[keep])):.3f} of 2 b, largest d rho {d[keep].max():.2e}')
    assert left <= 0.01, left                                      # on the reference alone
    assert np.all(d[keep] <= 2 * b[keep]), np.max(d[keep] / (2 * b[keep]))


def test_class_layer():
    """T5: erpac_batch is finalize_erpac of Plan.execute_erpac with device decim and with host decim, the window in
    full-rate samples; reuse; cross-channel indices; stats; EpochsWavelet.erpac's concatenated scale list and
    padding."""
    E, C = 5, 5
    own = np.arange(C)
    cross = (np.array([0, 2, 1]), np.array([2, 1, 1]))
    # device decim: n = 4096, decim 4, window in full-rate samples
    n, dtype = 4096, 'float32'
    x, _ = coupled_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype)
    win = (150, 4001)
    t0, t1, step, T = time_window(n, 4, win, True)
    assert (t0, t1, step, T) == (38, 1001, 1, 963)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, decim=4)
    try:
        sums = p.execute_erpac(x, None, PHASE, AMP, (t0, t1), step)
        csums = p.execute_erpac(x, cross, PHASE, AMP, (t0, t1), step)
    finally:
        p.close()
    for out in KINDS:
        want = finalize_erpac(out, *sums, own, own, E)
        got = w.erpac_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, window=win, decim=4)
        assert got.shape == (C, len(PHASE), len(AMP), T) and np.array_equal(got, want, equal_nan=True), out
        got = w.erpac_batch(x, None, phase=PHASE, amp=AMP, out=out, indices=cross, window=win, decim=4)     # reuse
        assert np.array_equal(got, finalize_erpac(out, *csums, *cross, E), equal_nan=True), out
    got = w.erpac_batch(x, FREQS, phase=PHASE, amp=AMP, out='erpac_sum', window=win, decim=4)
    for u, v in zip(got, sums):
        assert np.array_equal(u, v)
    st = w.plan_stats()[-1]
    assert st['reduce_path'] == L.NW_REDUCE_ERPAC and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_decim_kernel'
    assert w.erpac_batch(x, FREQS, reuse=False, phase=PHASE, amp=AMP).shape == (C, len(PHASE), len(AMP), n)   # circular
    assert w.plan_stats()[-1]['reduce_path'] == L.NW_REDUCE_ERPAC
    # host decim: the rocFFT engine has no device decimation: a full-rate plan, step = decim
    n, dtype = 1000, 'float64'
    x, _ = coupled_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype, engine='rocfft')
    win = (37, 990)
    t0, t1, step, T = time_window(n, 4, win, False)
    assert (t0, t1, step, T) == (40, 990, 4, 238)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, engine='rocfft')
    try:
        sums = p.execute_erpac(x, cross, PHASE, AMP, (t0, t1), step)
    finally:
        p.close()
    for out in KINDS:
        got = w.erpac_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, indices=cross, window=win, decim=4)
        assert got.shape == (3, len(PHASE), len(AMP), T) and np.array_equal(got, finalize_erpac(out, *sums, *cross, E)), out
    # EpochsWavelet: the two frequency lists concatenated, padding in seconds, channels picked by name
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)                 # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype, engine='rocfft'))
    sub = np.ascontiguousarray(x[:, :3])
    pf, af = [FREQS[i] for i in PHASE], [FREQS[i] for i in AMP]
    idx = ([2, 0], [0, 1])
    for method in KINDS:
        assert np.array_equal(ew.erpac(['a', 'b', 'c'], pf, af, method=method, padding=0.0371),
                              w.erpac_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, window=(37, n - 37))), method
        assert np.array_equal(ew.erpac(['a', 'b', 'c'], pf, af, method=method, indices=idx, padding=0.1, decim=4),
                              w.erpac_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, indices=idx, window=(100, 900),
                                            decim=4)), method
    assert np.array_equal(ew.erpac(['a', 'b', 'c'], pf, af), w.erpac_batch(sub, FREQS, phase=PHASE, amp=AMP))
    with pytest.raises(ValueError, match='padding'):
        ew.erpac(['a', 'b'], pf, af, padding=0.5)


# One call per form family and dtype, each with partial scale tiles (9 x 17 of 26 scales) and a tail sample tile.
# (tag, n, dtype, plan keywords, device decim, strict).  strict: the two builds' transform rows are bit for bit the
# same, so the sums must be too: measured, that holds for the fp64 chirp-z and rocFFT forms.  The debug builds of
# the fused, decimated and two-pass transform kernels (fp64 and fp32) and of every fp32 form round their rows
# otherwise, by an ulp or two of the compute dtype (presumably the checks change which products the compiler fuses
# into sums; not established), so there the sums of the two libraries cannot agree bit for bit and the debug library's sums are held to
# ITS OWN rows instead, T2's way -- as are the strict forms'.
T6_FAMILIES = (('fused', 1024, {}, 1), ('chirp', 1201, {}, 1), ('decim', 4096, {}, 4),
               ('rocfft', 1000, {'engine': 'rocfft'}, 1), ('twopass', 32768, {}, 1))
T6_FORMS = tuple((f'{tag}-{dt[-2:]}', n, dt, kw, decim, dt == 'float64' and tag in ('chirp', 'rocfft'))
                 for tag, n, kw, decim in T6_FAMILIES for dt in ('float64', 'float32'))
T6_PAIRS, T6_PH, T6_AM = (np.array([0, 1, 1]), np.array([0, 1, 0])), list(range(9)), list(range(9, 26))


def t6_call(n, dt, kw, decim):
    """(window, rows (3, 2, 26, n_out), sums) of one form on whichever library is loaded: chunks of 2 and 1 epochs.
    (Its source is also the debug child's: it uses the names np, nw and L alone.)"""
    x = np.random.default_rng(n).standard_normal((3, 2, n)).astype(dt)
    p = nw.Plan(n, 26, dt, max_batch=5, decim=decim, **kw)
    try:
        p.set_wavelet('morse', [17.5, 3.], np.geomspace(4., 300., 26), L.trans_grid(n / 1000., 1000., False))
        win = (5, min(p.n_out, 1206))
        sums = p.execute_erpac(x, ([0, 1, 1], [0, 1, 0]), list(range(9)), list(range(9, 26)), win)
        rows = p.execute(x.reshape(6, n), out_kind='cwt').reshape(3, 2, 26, p.n_out)
    finally:
        p.close()
    return win, rows, sums


T6_LOOP = ('for tag, n, dt, kw, decim, strict in %r:\n'
           '    win, rows, sums = t6_call(n, dt, kw, decim)\n'
           '    np.savez(%r %% tag, rows, *sums)\n'
           '    print("done", tag, sums[0].shape[-1] %% 64)\n')


def test_erpac_under_bounds_checks(tmp_path):
    """T6: the debug library (kernel bounds checks, nw_dcheck.h) on one call per form family in fp64 and in fp32: no
    check fails.  The values: on the strict forms (T6_FORMS) the two libraries' rows are bit for bit the same
    (asserted) and so are the sums (asserted); every form's sums, strict or not, are held to the debug library's
    own rows reduced in numpy in epoch order, as T2 does: sum (re^2 + im^2) array_equal, every other sum within
    1e-13 sum_e (A_{e,a}, A_{e,c}, 1); and wherever another form's rows happen to be the same, its sums are."""
    import inspect
    path = os.path.join(str(tmp_path), 'erpac_%s.npz')
    lines = run_under_bounds_checks(inspect.getsource(t6_call) + T6_LOOP % (T6_FORMS, path))
    ip, ia = T6_PAIRS
    failed = []
    for tag, n, dt, kw, decim, strict in T6_FORMS:
        assert any(ln.startswith(f'done {tag} ') and not ln.endswith(' 0') for ln in lines), lines    # a tail tile
        win, rows, sums = t6_call(n, dt, kw, decim)
        with np.load(path % tag) as z:
            drows, debug = z['arr_0'], [z[f'arr_{k}'] for k in (1, 2, 3)]
        for k, (u, v) in enumerate(zip(debug, sums)):
            assert u.shape == v.shape and u.dtype == v.dtype and np.all(np.isfinite(u)), (tag, k)
        same = np.array_equal(rows, drows)
        equal = all(np.array_equal(u, v) for u, v in zip(debug, sums))
        # the debug library's sums against its own rows
        y = drows.astype(np.complex128)
        idx = np.arange(*win)
        oM, oamp, ophase = own_sums(y, ip, ia, T6_PH, T6_AM, idx)
        sAc = np.max(np.abs(y), axis=(2, 3)).sum(0)
        power = np.array_equal(debug[1][..., 1], oamp[..., 1])
        dM = np.max(np.abs(debug[0] - oM) / sAc[ia][:, None, None, None])
        dA = np.max(np.abs(debug[1][..., 0] - oamp[..., 0]) / sAc[:, None, None])
        du = np.abs(debug[2] - ophase).max()
        apart = np.max(np.abs(drows.astype(np.complex128) - rows)) / np.max(np.abs(rows))
        print(f'{tag}: the two builds\' rows {"are bit for bit the same" if same else f"differ by {apart:.1e} of max |y|"}, their sums '
              f'{"are the same" if equal else "differ"}; against the debug rows: sum A^2 {"equal" if power else "NOT equal"}, '
              f'dM {dM:.2e} sum A_a, d sum A {dA:.2e} sum A_c, d phase sums {du:.2e} (bound {1e-13 * 3:.1e})')
        if strict and not (same and equal):
            failed.append((tag, 'rows' if not same else 'sums'))
        if same and not equal:
            failed.append((tag, 'the same rows, other sums'))
        if not power or dM > 1e-13 or dA > 1e-13 or du > 1e-13 * 3:
            failed.append((tag, 'own rows', power, dM, dA, du))
    assert not failed, failed
