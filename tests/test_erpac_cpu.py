"""Event-related phase-amplitude coupling without a GPU: the kernel's block map and tile geometry (nw_shape.h, a
stand-alone host program), the numpy finaliser engine.finalize_erpac against the formulas evaluated per sample
with np.corrcoef and against finalize_pac, its conventions, the argument checks of the plan-free layers that
fire before any device work, and the new constant, exports and signature."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FakeEpochs

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import ERPAC_OUTS, finalize_erpac, finalize_pac

SHARED = ('mvl', 'mvl_norm', 'direct_pac', 'debiased_pac')


def test_block_map_and_tile_geometry_on_the_host(tmp_path):
    """tests/asan/erpac_shape.cpp (a stand-alone program over nw_shape.h) under -fsanitize=address,undefined:
    one block per (pair, phase tile, amplitude tile, sample tile) in both block orders, the padding slots past
    the end, partial tiles (Fp = 9, Fa = 17, T in {0, 1, 63, 64, 65, 1201}) included."""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'erpac_shape')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'asan', 'erpac_shape.cpp'), '-o', exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def _sums(y, fph, fam, ip, ia):
    """The across-epoch sums of rows y (E, C, F, T), formed directly: (M, amp, phase, A (E, C, Fa, T), c, s
    (E, C, Fp, T))."""
    A = np.abs(y[:, :, fam])
    u = y[:, :, fph] / np.abs(y[:, :, fph])
    c, s = u.real, u.imag
    M = np.einsum('epit,epkt->pikt', u[:, ip], A[:, ia].astype(np.complex128))
    amp = np.stack([A.sum(0), (A * A).sum(0)], axis=-1)                           # (C, Fa, T, 2)
    phase = np.stack([c.sum(0), s.sum(0), (c * c).sum(0), (s * s).sum(0), (c * s).sum(0)], axis=2)   # (C, Fp, 5, T)
    return M, amp, phase, A, c, s


def _case():
    rng = np.random.default_rng(20)
    E, C, F, T = 12, 3, 7, 20
    y = rng.standard_normal((E, C, F, T)) + 1j * rng.standard_normal((E, C, F, T))
    fph, fam = np.array([0, 1, 1]), np.array([2, 6, 3, 2])                          # repeated list entries
    ip, ia = np.array([0, 2, 1, 1]), np.array([1, 0, 1, 2])
    return (E, C, F, T), y, fph, fam, ip, ia


def test_finalize_erpac_circular_against_corrcoef():
    (E, C, F, T), y, fph, fam, ip, ia = _case()
    M, amp, phase, A, c, s = _sums(y, fph, fam, ip, ia)
    rho = finalize_erpac('circular', M, amp, phase, ip, ia, E)
    assert rho.shape == (len(ip), len(fph), len(fam), T) and rho.dtype == np.float64
    want = np.empty_like(rho)
    for p in range(len(ip)):
        for i in range(len(fph)):
            for k in range(len(fam)):
                for t in range(T):
                    x, cc, ss = A[:, ia[p], k, t], c[:, ip[p], i, t], s[:, ip[p], i, t]
                    rxc, rxs, rcs = np.corrcoef(x, cc)[0, 1], np.corrcoef(x, ss)[0, 1], np.corrcoef(cc, ss)[0, 1]
                    want[p, i, k, t] = np.sqrt((rxc ** 2 + rxs ** 2 - 2 * rxc * rxs * rcs) / (1 - rcs ** 2))
    assert np.max(np.abs(rho - want)) <= 1e-12, np.max(np.abs(rho - want))
    assert rho.min() >= 0 and rho.max() <= 1 + 1e-12
    pval = finalize_erpac('circular_pval', M, amp, phase, ip, ia, E)
    assert np.array_equal(pval, np.exp(-E * rho * rho / 2.)) and pval.shape == rho.shape
    assert pval.min() > 0 and pval.max() <= 1
    # the repeated list entries give repeated cells
    assert np.array_equal(rho[:, 1], rho[:, 2]) and np.array_equal(rho[:, :, 0], rho[:, :, 3])


def test_finalize_erpac_shared_kinds_are_finalize_pac_on_the_moved_axes():
    (E, C, F, T), y, fph, fam, ip, ia = _case()
    M, amp, phase, A, c, s = _sums(y, fph, fam, ip, ia)
    assert set(SHARED) | {'erpac_sum', 'circular', 'circular_pval'} == set(ERPAC_OUTS)
    u = phase[:, :, 0] + 1j * phase[:, :, 1]                                      # (C, Fp, T)
    for kind in SHARED:
        got = finalize_erpac(kind, M, amp, phase, ip, ia, E)
        want = finalize_pac(kind, np.moveaxis(M, -1, 0), np.moveaxis(amp, 2, 0), np.moveaxis(u, -1, 0), ip, ia, E)
        assert got.shape == (len(ip), len(fph), len(fam), T) and got.dtype == np.float64 and got.flags.c_contiguous
        assert np.array_equal(got, np.moveaxis(want, 0, -1)), kind
    # ... which is the measure over the epochs: direct_pac per sample
    d = finalize_erpac('direct_pac', M, amp, phase, ip, ia, E)
    ref = np.abs(M) / np.sqrt(E * amp[ia][:, None, :, :, 1])
    assert np.allclose(d, ref, rtol=1e-12, atol=1e-14)
    got = finalize_erpac('erpac_sum', M, amp, phase, ip, ia, E)
    assert got[0] is M and got[1] is amp and got[2] is phase


def test_finalize_erpac_conventions():
    (E, C, F, T), y, fph, fam, ip, ia = _case()
    M, amp, phase, A, c, s = _sums(y, fph, fam, ip, ia)
    # a constant amplitude across the epochs has no variance: 0, not NaN (and p = 1)
    yc = y.copy()
    yc[:, 1, 6] = 3. * yc[:, 1, 6] / np.abs(yc[:, 1, 6])
    Mc, ampc, phasec = _sums(yc, fph, fam, ip, ia)[:3]
    # exact sums of a constant: sum A = 3 E and sum A^2 = 9 E whatever the rounding of |3 u|
    ampc[1, 1, :, 0], ampc[1, 1, :, 1] = 3. * E, 9. * E
    rho = finalize_erpac('circular', Mc, ampc, phasec, ip, ia, E)
    assert not np.any(rho[ia == 1][:, :, 1]) and np.all(np.isfinite(rho))
    assert np.all(finalize_erpac('circular_pval', Mc, ampc, phasec, ip, ia, E)[ia == 1][:, :, 1] == 1.)
    # c and s perfectly correlated (c = s = +-1/2, exact in binary, so that r_cs is exactly 1): 1 - r_cs^2 = 0 gives 0
    E2 = 6
    ph2 = np.zeros((1, 1, 5, 1))
    cs = np.array([1, -1, 1, -1, 1, -1]) / 2.
    ph2[0, 0, :, 0] = [cs.sum(), cs.sum(), (cs * cs).sum(), (cs * cs).sum(), (cs * cs).sum()]
    a2 = np.arange(1., 7.)
    amp2 = np.array([a2.sum(), (a2 * a2).sum()]).reshape(1, 1, 1, 2)
    M2 = np.array((a2 * cs).sum() * (1 + 1j)).reshape(1, 1, 1, 1)
    assert finalize_erpac('circular', M2, amp2, ph2, [0], [0], E2)[0, 0, 0, 0] == 0.
    # a NaN sum stays NaN, elsewhere nothing changes
    Mn, phn = M.copy(), phase.copy()
    phn[0, 0, :, 3] = np.nan
    Mn[ip == 0, 0, :, 3] = np.nan
    ref = finalize_erpac('circular', M, amp, phase, ip, ia, E)
    for kind in ('circular', 'circular_pval'):
        got = finalize_erpac(kind, Mn, amp, phn, ip, ia, E)
        assert np.all(np.isnan(got[ip == 0, 0, :, 3]))
        keep = np.ones(ref.shape, dtype=bool)
        keep[ip == 0, 0, :, 3] = False
        assert np.all(np.isfinite(got[keep]))
    assert np.array_equal(finalize_erpac('circular', Mn, amp, phn, ip, ia, E)[keep], ref[keep])
    # epoch counts
    for kind in ('circular', 'circular_pval'):
        for E0 in (1, 0):
            with pytest.raises(ValueError, match='at least 2 epochs'):
                finalize_erpac(kind, M, amp, phase, ip, ia, E0)
    for kind in SHARED:
        assert finalize_erpac(kind, M, amp, phase, ip, ia, 1).shape == M.shape
        with pytest.raises(ValueError, match='at least 1 epoch'):
            finalize_erpac(kind, M, amp, phase, ip, ia, 0)
    assert finalize_erpac('erpac_sum', M, amp, phase, ip, ia, 0)[0] is M
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_erpac('pac_sum', M, amp, phase, ip, ia, E)
    with pytest.raises(ValueError, match='phase'):
        finalize_erpac('circular', M, amp, phase[:, :, :2], ip, ia, E)
    # empty pair and sample axes keep their shapes
    for kind in SHARED + ('circular', 'circular_pval'):
        assert finalize_erpac(kind, M[:0], amp, phase, ip[:0], ia[:0], E).shape == (0, len(fph), len(fam), T)
        assert finalize_erpac(kind, M[..., :0], amp[:, :, :0], phase[..., :0], ip, ia, E).shape == M.shape[:3] + (0,)


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    freqs = [4., 7., 12., 40., 70.]
    w = nw.Morse(1000)
    ok = dict(phase=[0, 1], amp=[3, 4])
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.erpac_batch(x, freqs, decim=decim, **ok)
    for out in ('cwt', 'coherence', 'pac_sum', 'mi', None):                    # unknown out
        with pytest.raises(ValueError, match='out must be one of'):
            w.erpac_batch(x, freqs, out=out, **ok)
    with pytest.raises(TypeError):                                              # the epochs are already reduced
        w.erpac_batch(x, freqs, average=True, **ok)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.erpac_batch(bad, freqs, **ok)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.erpac_batch(x, freqs, indices=idx, **ok)
    for bad in ([5], [-1], [0, 7], [], None, [1.5]):                            # bad lists
        with pytest.raises(ValueError, match='phase'):
            w.erpac_batch(x, freqs, phase=bad, amp=[3, 4])
        with pytest.raises(ValueError, match='amp'):
            w.erpac_batch(x, freqs, phase=[0, 1], amp=bad)
    with pytest.raises(ValueError, match='phase'):                              # the defaults are no lists
        w.erpac_batch(x, freqs)
    for win in ((-1, 5), (6, 5), (0, 4097), (0.5, 3), (1,), 7):                 # bad window
        with pytest.raises(ValueError, match='window'):
            w.erpac_batch(x, freqs, window=win, **ok)
    for out in ('circular', 'circular_pval'):                                   # too few epochs
        with pytest.raises(ValueError, match='at least 2 epochs'):
            w.erpac_batch(x[:1], freqs, out=out, **ok)
    with pytest.raises(ValueError, match='at least 1 epochs'):
        w.erpac_batch(x[:0], freqs, out='mvl', **ok)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.erpac(['a', 'b'], [4., 7.], [40., 70.], decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.erpac(['a', 'b'], [4., 7.], [40., 70.], method='itc')
    with pytest.raises(ValueError, match='indices'):
        ew.erpac(['a', 'b'], [4., 7.], [40., 70.], indices=([0], [2]))
    with pytest.raises(ValueError):
        ew.erpac(['a', 'z'], [4., 7.], [40., 70.])                              # no such channel
    with pytest.raises(ValueError, match='phase'):
        ew.erpac(['a', 'b'], [], [40., 70.])
    with pytest.raises(ValueError, match='amp'):
        ew.erpac(['a', 'b'], [4., 7.], [])
    for padding in (2.048, 3., -0.1, float('nan')):
        with pytest.raises(ValueError, match='padding'):
            ew.erpac(['a', 'b'], [4., 7.], [40., 70.], padding=padding)
    assert w._cache is None and not w._plans


def test_constants_and_exports():
    assert L.NW_REDUCE_ERPAC == 8
    assert {L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS, L.NW_REDUCE_CONN, L.NW_REDUCE_CONN_TIME,
            L.NW_REDUCE_PAC, L.NW_REDUCE_ENV, L.NW_REDUCE_PAC_BINS, L.NW_REDUCE_ERPAC} == set(range(9))
    assert ERPAC_OUTS == {'erpac_sum', 'circular', 'circular_pval', 'mvl', 'mvl_norm', 'direct_pac', 'debiased_pac'}
    assert nw.finalize_erpac is finalize_erpac and 'finalize_erpac' in nw.__all__
    assert hasattr(nw.Plan, 'execute_erpac') and hasattr(nw.WaveletBase, 'erpac_batch') and hasattr(nw.EpochsWavelet, 'erpac')
    sig = {s[0]: s for s in L.SIGNATURES}
    assert 'nw_execute_erpac' in sig and sig['nw_execute_erpac'][1:] == sig['nw_execute_pac'][1:]
    assert len(sig['nw_execute_erpac'][2]) == 18
    with open(os.path.join(ROOT, 'include', 'ninwave.h')) as f:
        header = f.read()
    assert '#define NW_REDUCE_ERPAC 8' in header and 'int nw_execute_erpac(' in header
    assert hasattr(L.lib(), 'nw_execute_erpac')                   # the library exports it (host-only load)
