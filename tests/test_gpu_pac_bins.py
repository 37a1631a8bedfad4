"""GPU tests of phase-binned phase-amplitude coupling: nw_execute_pac_bins (nw_pac_bins_kernel and
nw_pac_bins_rows_kernel, nw_pac_bins.hip) through Plan.execute_pac_bins, engine.finalize_pac_bins,
WaveletBase.pac_bins_batch and EpochsWavelet.pac_bins.

For epoch e, a pair (p, a) of a phase and an amplitude channel with rows y_e,c (F, n_out), listed phase scales fph,
amplitude scales fam, nbins phase bins and a window of T samples s_j = t0 + j step:
    S = sum_{j : bin_j = b} |y_a[fa, s_j]| (E, P, Fp, Fa, nbins),   N = #{j : bin_j = b} (E, C, Fp, nbins),
bin_j the bin of y_p[fp, s_j] by the rule of ninwave.h (pac_bins_cases.bin_of).  References are formed here from
oracle.nw_oracle in complex128 with the same rule.

Inputs, scales, PAIRS, windows, tol and A_c are test_gpu_pac.py's (the coupled recipe of epoch_cases.py, E = 3, C = 5,
FREQS, phase = [0 .. 3], amp = [4 .. 8], max_batch = 2 C + 3); nbins = 18 unless stated.
u_j = min(2, 2 tol A_p / |y_p|); a sample is ambiguous at edge g when its oracle phase lies within (pi / 2) u_j of
theta_g (a chord |du| moves an angle by at most (pi / 2) |du|); bN_b = the samples ambiguous at edge b or b + 1 (cyclic).
  T1  against the oracle, every form and window: |N' - N| <= bN; |S' - S| <= 2 tol A_a (N + bN) + sum_{ambiguous at b
      or b + 1} |y_a| + 1e-13 T A_a.  On the reference alone, at n = 1024 and n = 1201 for the windows full and
      (37, 1001): the rule agrees with floor((atan2 + pi) / (2 pi / 18)) on every sample; the ambiguous samples are
      <= 3.5 % of the window in every (e, c, phase scale) and hold <= 5 % of sum |y_a| in every cell; no bin is empty; at
      the fp64 tol no sample is ambiguous; the epoch-averaged mi of the coupled cell (7 Hz, 70 Hz) of every even channel
      is >= 2 x the largest cell of the uncoupled channel 3.
  T2  the plan's own rows binned and summed in numpy in the contract's order: counts array_equal, S within
      1e-13 T A_a (hypot may differ in the last place); fp64 on every fp64 form, fp32 with max_batch = 2 C.
  T3  bit for bit, fp32 and fp64: any pair list, any scale lists, any max_batch, device tensors, no counts; the counts
      sum to T; nbins = 2's counts are the half-plane test of the plan's own rows (the one-chunk plan, so in fp32 too)
      and its sums those rows' magnitudes split by it; empty shapes; errors.
  T4  measures: fp64 every kind within 1e-7 of finalize_pac_bins on the oracle's sums (pref_phase equal); fp32: the
      planted coupling shows in the device's mi (no bound on mi against the oracle: the first-order worst case charges
      every ambiguous sample as flipped and comes out at 40 .. 100 x the measure); max |d mi| is printed.
  T5  the layers; T6 the debug library."""
import numpy as np
import pytest

from epoch_cases import (FREQS, OVER_TIME, FakeEpochs, forms, morse_plan, run_under_bounds_checks, tol_of, windows_of)
from epoch_cases import coupled_rows as oracle_rows
from pac_bins_cases import atan2_bin, bin_of, binned_sums

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import finalize_pac_bins, time_window  # noqa: E402

PHASE, AMP = [0, 1, 2, 3], [4, 5, 6, 7, 8]
FREQS3 = [7., 70., 200.]             # this file's three: the coupled pair of scales is among them
FREQS26 = [float(f) for f in np.round(np.geomspace(4., 300., 26), 2)]
KINDS = ('bin_amp', 'mi', 'hr', 'pref_phase')
NBINS = 18
# (phase channel, amplitude channel): every channel with itself, then three cross-channel pairs
PAIRS = (np.array([0, 1, 2, 3, 4, 0, 1, 2]), np.array([0, 1, 2, 3, 4, 2, 0, 3]))
UNCOUPLED = 3                        # the uncoupled channel of the planted-coupling check


def pairs_of(C):
    ip, ia = PAIRS
    keep = (ip < C) & (ia < C)
    return ip[keep], ia[keep]


def ambiguous(y, fph, idx, Ac, tol, nbins):
    """(E, C, Fp, T, nbins) bool: the oracle phase of the sample lies within (pi / 2) u_j of edge g."""
    yp = y[:, :, fph][..., idx]
    with np.errstate(divide='ignore'):
        u = np.minimum(2., 2 * tol * Ac[:, :, None, None] / np.abs(yp))
    theta = -np.pi + 2 * np.pi * np.arange(nbins) / nbins
    d = np.angle(yp)[..., None] - theta
    d = np.abs((d + np.pi) % (2 * np.pi) - np.pi)                                  # the distance on the circle
    return d <= (np.pi / 2) * u[..., None]


def planted(mi, fph, fam):
    """(the coupled cell (7 Hz, 70 Hz) of the even channels, the largest cell of the uncoupled channel) of an
    epoch-averaged own-channel mi (C, Fp, Fa)."""
    return mi[0::2, fph.index(1), fam.index(5)], mi[UNCOUPLED].max()


def check_reference(name, y, fph, fam, idx, Ac, tol, dtype):
    """On the reference alone, nbins = 18."""
    T = len(idx)
    C = y.shape[1]
    own = np.arange(C)
    ip, ia = pairs_of(C)
    rS, rN, bins, A = binned_sums(y, ip, ia, fph, fam, idx, NBINS, False)
    yp = y[:, :, fph][..., idx]
    assert np.array_equal(bins, atan2_bin(yp.real, yp.imag, NBINS)), name
    amb = ambiguous(y, fph, idx, Ac, tol, NBINS).any(axis=-1)                      # (E, C, Fp, T)
    frac = amb.mean(axis=-1)
    share = np.einsum('epit,epkt->epik', amb[:, ip].astype(np.float64), A[:, ia]) / A[:, ia].sum(-1)[:, :, None, :]
    mi = finalize_pac_bins('mi', rS[:, :C], rN, own).mean(axis=0)                  # PAIRS starts with the own pairs
    coupled, other = planted(mi, fph, fam)
    print(f'{name} T={T}: reference: ambiguous <= {frac.max():.4f} of the window, <= {share.max():.4f} of sum |y_a|, '
          f'smallest count {int(rN.min())}, coupled mi {coupled.min():.4f} .. {coupled.max():.4f}, channel {UNCOUPLED} '
          f'<= {other:.4f}')
    assert frac.max() <= 0.035 and share.max() <= 0.05, (name, frac.max(), share.max())
    assert rN.min() >= 1, name
    if dtype == 'float64':
        assert not amb.any(), name
    assert coupled.min() >= 2 * other, (name, coupled.min(), other)


def check_t1(name, got, y, Ac, ip, ia, fph, fam, idx, tol, nbins):
    """T1 of (S, N) over the window samples ``idx`` (indices into the reference rows); returns the reference's."""
    S, N = got
    T = len(idx)
    rS, rN, _, A = binned_sums(y, ip, ia, fph, fam, idx, nbins, False)
    assert S.shape == rS.shape and N.shape == rN.shape, name
    amb = ambiguous(y, fph, idx, Ac, tol, nbins)
    amb = amb | np.roll(amb, -1, axis=-1)                                          # at edge b or b + 1
    bN = amb.sum(axis=3).astype(np.float64)                                        # (E, C, Fp, nbins)
    Aa = Ac[:, ia][:, :, None, None, None]
    bS = (2 * tol * Aa * (rN + bN)[:, ip][:, :, :, None, :]
          + np.einsum('epitb,epkt->epikb', amb[:, ip].astype(np.float64), A[:, ia]) + 1e-13 * T * Aa)
    dN, dS = np.abs(N - rN), np.abs(S - rS)
    print(f'{name} T1: dS {np.max(dS / bS):.3f} of its bound; dN up to {int(dN.max())}, {np.max(dN - bN):.0f} over its '
          f'bound (largest bound {int(bN.max())})')
    assert np.all(dN <= bN), (name, np.max(dN - bN))
    assert np.all(dS <= bS), (name, np.max(dS / bS))
    return rS, rN


# (id, n, dtype, E, C, freqs, phase, amp, nbins, plan keywords, device decim, host decim, kernel of the form)
CASES = []
for name, n, dtype, kw, decim, host_decim, kernel in forms(*OVER_TIME[:-1]):
    E, C, freqs, fph, fam = (2, 3, FREQS3, [0], [1, 2]) if name == 'twopass-32768' else (3, 5, FREQS, PHASE, AMP)
    CASES.append((name, n, dtype, E, C, freqs, fph, fam, NBINS, kw, decim, host_decim, kernel))
# 9 phase x 17 amplitude scales: nine phase positions and three amplitude tiles of eight, the last one partial
CASES.append(('tiles-9x17-f64', 1024, 'float64', 2, 2, FREQS26, list(range(9)), list(range(9, 26)), NBINS, {}, 1, 1,
              'nw_fused_kernel'))
# the other two geometry classes: 16 and 4 amplitude scales per tile
for nb in (4, 36):
    CASES.append((f'1024-f64-{nb}bins', 1024, 'float64', 3, 5, FREQS, PHASE, AMP, nb, {}, 1, 1, 'nw_fused_kernel'))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 for every case and window, T2 for the fp64 cases; PAIRS; max_batch = 2 C + 3."""
    name, n, dtype, E, C, freqs, fph, fam, nbins, kw, decim, host_decim, kernel = case
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
            got[wname] = (win, step, p.execute_pac_bins(x, (ip, ia), fph, fam, win, step, nbins))
            st = p.stats()
            assert st['reduce_path'] == L.NW_REDUCE_PAC_BINS and L.KERNEL_NAMES[st['kernel']] == kernel, (name, st)
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
        S, N = sums
        assert S.dtype == np.float64 and N.dtype == np.float64
        assert S.shape == (E, len(ip), len(fph), len(fam), nbins) and N.shape == (E, C, len(fph), nbins)
        if T == 0:                                             # an empty window: zero sums
            assert not np.any(S) and not np.any(N), (name, wname)
            continue
        assert np.array_equal(N.sum(axis=-1), np.full((E, C, len(fph)), float(T))), (name, wname)
        if n in (1024, 1201) and freqs is FREQS and nbins == NBINS and wname in ('full', 'inner'):
            check_reference(f'{name} {wname}', y, fph, fam, idx, Ac, tol, dtype)
        check_t1(f'{name} {wname}', sums, y, Ac, ip, ia, fph, fam, idx * decim, tol, nbins)
        if rows is not None:                                   # T2
            oS, oN, _, _ = binned_sums(rows, ip, ia, fph, fam, idx, nbins, True)
            assert np.array_equal(N, oN), (name, wname, np.abs(N - oN).max())
            dS = np.max(np.abs(S - oS) / Ac[:, ia][:, :, None, None, None])
            print(f'{name} {wname} T2: counts equal; dS {dS:.2e} A_a (bound {1e-13 * T:.1e})')
            assert dS <= 1e-13 * T, (name, wname, dS)


@pytest.mark.parametrize('form', ['1024-f32', 'chirp-1201-f32'])
def test_fp32_sums_are_the_plans_own_rows_binned(form):
    """T2 in fp32: max_batch = 2 C, so that execute(cwt) on (E C, n) chunks the same signals together."""
    (name, n, dtype, kw, _, _, _), = forms(form)
    E, C = 3, 5
    x, y = oracle_rows(n, E, C, dtype, FREQS)
    Ac = np.max(np.abs(y), axis=(2, 3))
    ip, ia = pairs_of(C)
    p = morse_plan(n, dtype, FREQS, 2 * C, **kw)
    try:
        got = {win: p.execute_pac_bins(x, (ip, ia), PHASE, AMP, win, step, NBINS)
               for win, step in (((0, n), 1), ((37, 1001), 1), ((5, n - 3), 4))}
        rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, len(FREQS), n)
    finally:
        p.close()
    for win, (S, N) in got.items():
        idx = np.arange(win[0], win[1], 4 if win[0] == 5 else 1)
        oS, oN, _, _ = binned_sums(rows, ip, ia, PHASE, AMP, idx, NBINS, True)
        assert np.array_equal(N, oN), (name, win, np.abs(N - oN).max())
        dS = np.max(np.abs(S - oS) / Ac[:, ia][:, :, None, None, None])
        print(f'{name} {win} T2: counts equal; dS {dS:.2e} A_a (bound {1e-13 * len(idx):.1e})')
        assert dS <= 1e-13 * len(idx), (name, win, dS)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_a_cells_sums_depend_only_on_its_rows_nbins_and_the_window(dtype):
    """T3, bit for bit: any pair list; any scale lists; any chunking; the counts."""
    n, E, C = 1024, 3, 5
    x, y = oracle_rows(n, E, C, dtype, FREQS)
    Ac = np.max(np.abs(y), axis=(2, 3))
    ip, ia = pairs_of(C)
    win = (37, 1001)
    T = win[1] - win[0]
    la, lb = np.array([4, 0, 3, 2, 2, 0, 1]), np.array([4, 2, 3, 3, 3, 2, 0])      # shuffled, repeated, cross, own
    sph, sam = [3, 1, 1, 5, 0], [5, 8, 4, 4, 1, 6, 7]            # reordered, repeated, 5 and 1 in both lists
    res = {}
    for mb in (C, 2 * C + 3, E * C):
        p = morse_plan(n, dtype, FREQS, mb)
        try:
            res[mb] = p.execute_pac_bins(x, (ip, ia), PHASE, AMP, win)            # nbins = 18 by default
            assert p.stats()['chunks'] == -(-E // (mb // C))
            if mb == 2 * C + 3:
                lst = p.execute_pac_bins(x, (la, lb), PHASE, AMP, win, 1, NBINS)
                scl = p.execute_pac_bins(x, (ip, ia), sph, sam, win, 1, NBINS)
                own = p.execute_pac_bins(x, None, PHASE, AMP, win, 1, NBINS)
                amp = p.execute_pac(x, None, PHASE, AMP, win)[1]
            if mb == E * C:      # one chunk: execute on (E C, n) transforms the same signals together, in fp32 too
                two = p.execute_pac_bins(x, None, PHASE, AMP, win, 1, 2)
                rows = p.execute(x.reshape(E * C, n), out_kind='cwt').astype(np.complex128).reshape(E, C, len(FREQS), n)
        finally:
            p.close()
    S, N = res[2 * C + 3]
    assert S.shape == (E, len(ip), len(PHASE), len(AMP), NBINS) and N.shape == (E, C, len(PHASE), NBINS)
    for mb in (C, E * C):                                         # any chunking
        for u, v in zip(res[mb], res[2 * C + 3]):
            assert np.array_equal(u, v), mb
    # the counts are whole numbers and every row of them is the window
    assert np.array_equal(N, np.round(N)) and N.min() >= 0 and np.array_equal(N.sum(-1), np.full(N.shape[:-1], float(T)))
    # indices=None: every channel with itself
    assert np.array_equal(own[0], S[:, :C]) and np.array_equal(own[1], N)
    # any pair list
    assert np.array_equal(lst[1], N)
    for k, (a, b) in enumerate(zip(la, lb)):
        q = int(np.flatnonzero((ip == a) & (ia == b))[0])
        assert np.array_equal(lst[0][:, k], S[:, q]), (a, b)
    # any scale lists: a cell is its (phase scale, amplitude scale)'s, wherever it stands
    sS, sN = scl
    assert sS.shape == (E, len(ip), len(sph), len(sam), NBINS)
    for i, fp in enumerate(sph):
        for k, fa in enumerate(sam):
            if fp in PHASE and fa in AMP:
                assert np.array_equal(sS[:, :, i, k], S[:, :, PHASE.index(fp), AMP.index(fa)]), (fp, fa)
        if fp in PHASE:
            assert np.array_equal(sN[:, :, i], N[:, :, PHASE.index(fp)]), fp
    assert np.array_equal(sS[:, :, 1], sS[:, :, 2]) and np.array_equal(sS[:, :, :, 2], sS[:, :, :, 3])   # the repeats
    # nbins = 2, fp32 and fp64: the counts are the half-plane test of the plan's own rows, bit for bit, and the two
    # sums are those rows' magnitudes split by it, in the contract's order (T2's bound: hypot's last place)
    yw = rows[:, :, PHASE, win[0]:win[1]]
    upper = (yw.imag > 0) | ((yw.imag == 0) & (yw.real > 0))
    assert two[0].shape == (E, C, len(PHASE), len(AMP), 2) and two[1].shape == (E, C, len(PHASE), 2)
    assert np.array_equal(two[1][..., 1], upper.sum(-1)) and np.array_equal(two[1][..., 0], T - upper.sum(-1))
    own2 = np.arange(C)
    oS, oN, _, _ = binned_sums(rows, own2, own2, PHASE, AMP, np.arange(*win), 2, True)
    assert np.array_equal(two[1], oN)
    dS = np.max(np.abs(two[0] - oS) / Ac[:, :, None, None, None])
    assert dS <= 1e-13 * T, dS
    # the bins of a cell partition the window: their sums add up to nw_execute_pac's sum A within rounding
    tot = amp[:, ia][:, :, None, :, 0]                            # (E, P, 1, Fa)
    assert np.allclose(S.sum(-1), np.broadcast_to(tot, S.shape[:-1]), rtol=1e-12, atol=0)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_device_tensors_edge_cases_and_errors(dtype):
    """T3: device tensors equal the host call, with and without the counts; empty window, E = 0, P = 0; bad
    arguments raise and the plan still works; execute_pac on the same plan is what it was."""
    import torch
    n, E, C = 1024, 3, 5
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    ip, ia = pairs_of(C)
    P, Fp, Fa = len(ip), len(PHASE), len(AMP)
    win = (37, 1001)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        pac_before = p.execute_pac(x, (ip, ia), PHASE, AMP, win)
        host = p.execute_pac_bins(x, (ip, ia), PHASE, AMP, win, 1, NBINS)
        tx = torch.from_numpy(np.array(x)).cuda()
        tS = torch.full((E, P, Fp, Fa, NBINS), float('nan'), dtype=torch.float64, device='cuda')
        tN = torch.full((E, C, Fp, NBINS), float('nan'), dtype=torch.float64, device='cuda')
        out = p.execute_pac_bins(tx, (ip, ia), PHASE, AMP, win, 1, NBINS, out=(tS, tN))
        assert out[0] is tS and out[1] is tN
        for t, h in zip((tS, tN), host):
            assert np.array_equal(t.cpu().numpy(), h)
        tS2 = torch.full((E, P, Fp, Fa, NBINS), float('nan'), dtype=torch.float64, device='cuda')
        p.execute_pac_bins(tx, (ip, ia), PHASE, AMP, win, 1, NBINS, out=(tS2, None))   # out_count = NULL
        assert np.array_equal(tS2.cpu().numpy(), host[0])
        # host output arrays are filled in place; window=None is the whole row
        mine = (np.empty((E, P, Fp, Fa, NBINS)), None)
        got = p.execute_pac_bins(x, (ip, ia), PHASE, AMP, win, out=mine)
        assert got[0] is mine[0] and np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
        full = p.execute_pac_bins(x, (ip, ia), PHASE, AMP)
        for u, v in zip(full, p.execute_pac_bins(x, (ip, ia), PHASE, AMP, (0, n))):
            assert np.array_equal(u, v)
        # an empty window: zero sums; no epochs, no pairs: empty outputs
        for a in p.execute_pac_bins(x, (ip, ia), PHASE, AMP, (n, n)):
            assert not np.any(a) and a.shape[0] == E
        z = p.execute_pac_bins(x[:0], (ip, ia), PHASE, AMP, win)
        assert z[0].shape == (0, P, Fp, Fa, NBINS) and z[1].shape == (0, C, Fp, NBINS)
        z = p.execute_pac_bins(x, ([], []), PHASE, AMP, win)
        assert z[0].shape == (E, 0, Fp, Fa, NBINS) and np.array_equal(z[1], host[1])
        assert p.stats()['reduce_path'] == L.NW_REDUCE_PAC_BINS
        # errors
        for bad in (0, 1, 3, 17, 38, -2, 2.5, None, '18', True):
            with pytest.raises(ValueError, match='nbins'):
                p.execute_pac_bins(x, None, PHASE, AMP, nbins=bad)
        for bad in ((-1, 5), (6, 5), (0, n + 1), (0.5, 3), (1,), 7):
            with pytest.raises(ValueError, match='window'):
                p.execute_pac_bins(x, None, PHASE, AMP, bad)
        for step in (0, -1, 1.5):
            with pytest.raises(ValueError, match='step'):
                p.execute_pac_bins(x, None, PHASE, AMP, step=step)
        for bad in ([9], [-1], [], None, [0.5]):
            with pytest.raises(ValueError, match='phase'):
                p.execute_pac_bins(x, None, bad, AMP)
            with pytest.raises(ValueError, match='amp'):
                p.execute_pac_bins(x, None, PHASE, bad)
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_pac_bins(x, (ip, ia), PHASE, AMP, out=(np.empty((E, P, Fp, Fa, NBINS), dtype=np.float32), None))
        with pytest.raises(ValueError, match='right dtype and size'):
            p.execute_pac_bins(x, (ip, ia), PHASE, AMP, out=(None, np.empty((E, C, Fp))))
        with pytest.raises(ValueError, match='indices'):
            p.execute_pac_bins(x, ([0], [C]), PHASE, AMP)
        with pytest.raises(ValueError, match='epochs, channels'):
            p.execute_pac_bins(x.reshape(E * C, n), None, PHASE, AMP)
        with pytest.raises(ValueError, match='output'):
            p.execute_pac_bins(tx, (ip, ia), PHASE, AMP)
        with pytest.raises(ValueError, match='float64'):
            p.execute_pac_bins(tx, (ip, ia), PHASE, AMP, out=(tS.to(torch.float32), tN))
        with pytest.raises(ValueError, match='hold'):
            p.execute_pac_bins(tx, (ip, ia), PHASE, AMP, out=(tS[:2], tN))
        with pytest.raises(ValueError, match='S, count'):
            p.execute_pac_bins(tx, (ip, ia), PHASE, AMP, out=tS)
        # the C ABI's own checks: nbins, and a scale position outside the plan's list
        import ctypes
        V_ = ctypes.c_void_p
        xc = np.ascontiguousarray(x)
        ii = ip.astype(np.int32)
        badf, okf = np.array([0, 9], dtype=np.int32), np.array([4, 5], dtype=np.int32)
        buf = np.empty((E, P, 2, 2, 38))

        def call(fa_, fb_, nb):
            return L.lib().nw_execute_pac_bins(p.handle, xc.ctypes.data_as(V_), E, C, ii.ctypes.data_as(V_),
                                               ii.ctypes.data_as(V_), len(ii), fa_.ctypes.data_as(V_), 2,
                                               fb_.ctypes.data_as(V_), 2, 0, n, 1, nb, buf.ctypes.data_as(V_), None,
                                               L.NW_MEM_HOST)
        for fa_, fb_, nb, word in ((badf, okf, 18, b'phase scale 1 = 9'), (okf, badf, 18, b'amplitude scale 1 = 9'),
                                   (okf, okf, 17, b'nbins (17)'), (okf, okf, 0, b'nbins (0)'), (okf, okf, 38, b'nbins (38)')):
            assert call(fa_, fb_, nb) == L.NW_E_INVALID and word in L.lib().nw_last_error(), L.lib().nw_last_error()
        assert call(okf, okf, 36) == L.NW_OK
        small = morse_plan(n, dtype, FREQS, C - 1)
        try:
            with pytest.raises(ValueError, match='max_batch'):
                small.execute_pac_bins(x, None, PHASE, AMP)
        finally:
            small.close()
        again = p.execute_pac_bins(x, (ip, ia), PHASE, AMP, win)                      # the plan still works
        for u, v in zip(again, host):
            assert np.array_equal(u, v)
        # ... and execute_pac on the same plan is what it was
        for u, v in zip(p.execute_pac(x, (ip, ia), PHASE, AMP, win), pac_before):
            assert np.array_equal(u, v)
        assert p.stats()['reduce_path'] == L.NW_REDUCE_PAC
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
    idx = np.arange(*win)
    rS, rN, _, _ = binned_sums(y, ip, ia, PHASE, AMP, idx, NBINS, False)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3)
    try:
        S, N = p.execute_pac_bins(x, (ip, ia), PHASE, AMP, win, 1, NBINS)
    finally:
        p.close()
    dmi = np.abs(finalize_pac_bins('mi', S, N, ip) - finalize_pac_bins('mi', rS, rN, ip)).max()
    print(f'n={n} {win} {dtype}: max |d mi| against the oracle {dmi:.3e}')
    if dtype == 'float64':
        for kind in KINDS:
            a, b = finalize_pac_bins(kind, S, N, ip), finalize_pac_bins(kind, rS, rN, ip)
            assert a.shape == b.shape and not np.isnan(a).any(), kind
            if kind == 'pref_phase':
                assert np.array_equal(a, b), kind
            else:
                assert np.abs(a - b).max() <= 1e-7, (kind, np.abs(a - b).max())
        return
    mi = finalize_pac_bins('mi', S[:, :C], N, np.arange(C)).mean(axis=0)           # the device's, own pairs
    coupled, other = planted(mi, PHASE, AMP)
    print(f'n={n} {win} fp32: coupled mi {coupled.min():.4f} .. {coupled.max():.4f}, channel {UNCOUPLED} <= {other:.4f}')
    assert coupled.min() >= 2 * other, (coupled.min(), other)


def test_class_layer():
    """T5: pac_bins_batch is finalize_pac_bins of Plan.execute_pac_bins, with device decim and with host decim;
    average; cross-channel indices; EpochsWavelet.pac_bins's concatenated scale list, padding and names."""
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
        sums = p.execute_pac_bins(x, None, PHASE, AMP, (t0, t1), step, NBINS)
        csums = p.execute_pac_bins(x, cross, PHASE, AMP, (t0, t1), step, 12)
    finally:
        p.close()
    for out in KINDS:
        want = finalize_pac_bins(out, *sums, own)
        got = w.pac_bins_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, window=win, decim=4)
        assert got.shape == (E, C, len(PHASE), len(AMP)) + ((NBINS,) if out == 'bin_amp' else ())
        assert np.array_equal(got, want, equal_nan=True), out
        if out != 'pref_phase':
            avg = w.pac_bins_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, window=win, decim=4, average=True)
            assert avg.shape == got.shape[1:] and np.array_equal(avg, want.mean(axis=0), equal_nan=True), out
        got = w.pac_bins_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, nbins=12, indices=cross, window=win, decim=4)
        assert np.array_equal(got, finalize_pac_bins(out, *csums, cross[0]), equal_nan=True), out
    got = w.pac_bins_batch(x, FREQS, phase=PHASE, amp=AMP, out='bin_sum', window=win, decim=4)
    for u, v in zip(got, sums):
        assert np.array_equal(u, v)
    assert w.pac_bins_batch(x, FREQS, phase=PHASE, amp=AMP).shape == (E, C, len(PHASE), len(AMP))     # mi
    st = w.plan_stats()[-1]                                        # the most recent plan: the full-rate one
    assert st['reduce_path'] == L.NW_REDUCE_PAC_BINS
    # host decim: the rocFFT engine has no device decimation: a full-rate plan, step = decim
    n, dtype = 1000, 'float64'
    x, _ = oracle_rows(n, E, C, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype, engine='rocfft')
    win = (37, 990)
    t0, t1, step, T = time_window(n, 4, win, False)
    assert (t0, t1, step, T) == (40, 990, 4, 238)
    p = morse_plan(n, dtype, FREQS, 2 * C + 3, engine='rocfft')
    try:
        sums = p.execute_pac_bins(x, cross, PHASE, AMP, (t0, t1), step, 6)
    finally:
        p.close()
    for out in KINDS:
        got = w.pac_bins_batch(x, FREQS, phase=PHASE, amp=AMP, out=out, nbins=6, indices=cross, window=win, decim=4)
        assert np.array_equal(got, finalize_pac_bins(out, *sums, cross[0]), equal_nan=True), out
    # EpochsWavelet: the two frequency lists concatenated, padding in seconds, channels picked by name
    data = np.stack([x[:, 0], x[:, 4], x[:, 1], x[:, 2]], axis=1)                 # epochs channels a, x, b, c
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'x', 'b', 'c']), nw.Morse(1000, dtype=dtype, engine='rocfft'))
    sub = np.ascontiguousarray(x[:, :3])
    pf, af = [FREQS[i] for i in PHASE], [FREQS[i] for i in AMP]
    idx = ([2, 0], [0, 1])
    for method in KINDS:
        assert np.array_equal(ew.pac_bins(['a', 'b', 'c'], pf, af, method=method, padding=0.0371),
                              w.pac_bins_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, window=(37, n - 37)),
                              equal_nan=True), method
        avg = method != 'pref_phase'
        assert np.array_equal(ew.pac_bins(['a', 'b', 'c'], pf, af, method=method, nbins=8, indices=idx, padding=0.1,
                                          decim=4, average=avg),
                              w.pac_bins_batch(sub, FREQS, phase=PHASE, amp=AMP, out=method, nbins=8, indices=idx,
                                               window=(100, 900), decim=4, average=avg), equal_nan=True), method
    assert np.array_equal(ew.pac_bins(['a', 'b', 'c'], pf, af), w.pac_bins_batch(sub, FREQS, phase=PHASE, amp=AMP))
    with pytest.raises(ValueError, match='padding'):
        ew.pac_bins(['a', 'b'], pf, af, padding=0.5)


def test_pac_bins_under_bounds_checks():
    """T6: the debug library (kernel bounds checks, nw_dcheck.h) on n = 1024 fp32, on a tail tile (n = 1201 fp64) and
    on partial amplitude tiles (9 x 17 scales), nbins 2 / 18 / 36 (the three geometry classes), five windows, own and
    cross-channel pairs: no check fails, and every row of counts is the window."""
    body = ('rng = np.random.default_rng(1)\n'
            'for tag, n, E, C, dt, F, ph, am in (("a", 1024, 3, 5, "float32", 9, [0, 1, 2, 3], [4, 5, 6, 7, 8]),\n'
            '                                    ("b", 1201, 3, 5, "float64", 3, [0], [1, 2]),\n'
            '                                    ("c", 1024, 2, 2, "float64", 26, list(range(9)), list(range(9, 26)))):\n'
            '    x = rng.standard_normal((E, C, n)).astype(dt)\n'
            '    p = nw.Plan(n, F, dt, max_batch=2 * C + 3)\n'
            '    p.set_wavelet("morse", [17.5, 3.], np.geomspace(3., 300., F), L.trans_grid(n / 1000., 1000., False))\n'
            '    ok = True\n'
            '    for nb in (2, 18, 36):\n'
            '        for win, step in ((None, 1), ((37, 1001), 1), ((0, 1), 1), ((5, n), 4), ((9, 9), 1)):\n'
            '            T = L.conn_time_count(n, *(win or (0, n)), step)\n'
            '            own = p.execute_pac_bins(x, None, ph, am, win, step, nb)\n'
            '            short = p.execute_pac_bins(x, ([C - 1, 0, 1], [0, 0, 1]), am[:1] + ph, ph[:1] + am, win, step, nb)\n'
            '            for a in own + short:\n'
            '                ok = ok and bool(np.all(np.isfinite(a))) and a.shape[0] == E and a.shape[-1] == nb\n'
            '            ok = ok and bool(np.all(own[1].sum(-1) == T)) and bool(np.all(short[1].sum(-1) == T))\n'
            '    print("ok", tag, ok)\n'
            '    p.close()\n')
    lines = run_under_bounds_checks(body)
    assert 'ok a True' in lines and 'ok b True' in lines and 'ok c True' in lines, lines
