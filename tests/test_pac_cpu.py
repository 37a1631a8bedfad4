"""Phase-amplitude coupling without a GPU: the numpy finaliser engine.finalize_pac against direct formulas
for every kind, the kernel's block map and scale-tile geometry (nw_shape.h, a stand-alone host program), the
argument checks of the plan-free layers that fire before any device work, and the new constant, exports
and signature."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FakeEpochs

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import PAC_OUTS, check_pac_indices, check_scales, finalize_pac

KINDS = ('mvl', 'mvl_norm', 'direct_pac', 'debiased_pac')


def test_block_map_and_tile_geometry_on_the_host(tmp_path):
    """tests/asan/pac_shape.cpp (a stand-alone program over nw_shape.h) under -fsanitize=address,undefined:
    one block per (epoch, pair, phase tile, amplitude tile) in both block orders and every listed scale
    combination in exactly one tile, partial tiles (Fp = 9, Fa = 17) included."""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'pac_shape')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'asan', 'pac_shape.cpp'), '-o', exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def _sums(rng, E, C, F, T, fph, fam, ip, ia):
    """PAC sums of random rows (E, C, F, T), formed directly."""
    y = rng.standard_normal((E, C, F, T)) + 1j * rng.standard_normal((E, C, F, T))
    A = np.abs(y[:, :, fam])                                      # (E, C, Fa, T)
    u = y[:, :, fph] / np.abs(y[:, :, fph])                       # (E, C, Fp, T)
    M = np.einsum('epit,epkt->epik', u[:, ip], A[:, ia].astype(np.complex128))
    amp = np.stack([A.sum(-1), (A * A).sum(-1)], axis=-1)
    phase = u.sum(-1)
    return M, amp, phase, A, u


def test_finalize_pac_against_direct_formulas():
    rng = np.random.default_rng(11)
    E, C, F, T = 3, 3, 7, 50
    fph, fam = np.array([0, 1, 1]), np.array([2, 6, 3, 2])
    ip, ia = np.array([0, 2, 1, 1]), np.array([1, 0, 1, 2])
    M, amp, phase, A, u = _sums(rng, E, C, F, T, fph, fam, ip, ia)
    sA = amp[:, ia][:, :, None, :, 0]
    sA2 = amp[:, ia][:, :, None, :, 1]
    su = phase[:, ip][:, :, :, None]
    want = {'mvl': np.abs(M) / T, 'mvl_norm': np.abs(M) / sA, 'direct_pac': np.abs(M) / np.sqrt(T * sA2),
            'debiased_pac': np.abs(M - su * sA / T) / T}
    assert set(want) | {'pac_sum'} == set(PAC_OUTS)
    for kind, ref in want.items():
        got = finalize_pac(kind, M, amp, phase, ip, ia, T)
        assert got.shape == (E, len(ip), len(fph), len(fam)) and got.dtype == np.float64, kind
        assert np.allclose(got, ref, rtol=1e-12, atol=1e-14), kind
    # the debiased measure is the modulus of the mean of A (u - mean u)
    direct = np.abs(np.einsum('epit,epkt->epik', u[:, ip] - u[:, ip].mean(-1, keepdims=True),
                              A[:, ia].astype(np.complex128))) / T
    assert np.allclose(finalize_pac('debiased_pac', M, amp, phase, ip, ia, T), direct, rtol=1e-10, atol=1e-13)
    # direct_pac lies in [0, 1] (Cauchy-Schwarz)
    d = finalize_pac('direct_pac', M, amp, phase, ip, ia, T)
    assert d.min() >= 0 and d.max() <= 1 + 1e-12
    # the sums pass through unchanged
    got = finalize_pac('pac_sum', M, amp, phase, ip, ia, T)
    assert got[0] is M and got[1] is amp and got[2] is phase
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_pac('coherence', M, amp, phase, ip, ia, T)
    for kind in KINDS:
        for T0 in (0, -1):
            with pytest.raises(ValueError, match='at least 1'):
                finalize_pac(kind, M, amp, phase, ip, ia, T0)
    assert finalize_pac('pac_sum', M, amp, phase, ip, ia, 0)[0] is M
    # empty epoch and pair axes keep their shapes
    for kind in KINDS:
        assert finalize_pac(kind, M[:0], amp[:0], phase[:0], ip, ia, T).shape == (0, len(ip), len(fph), len(fam))
        assert finalize_pac(kind, M[:, :0], amp, phase, ip[:0], ia[:0], T).shape == (E, 0, len(fph), len(fam))


def test_finalize_pac_zero_denominators():
    E, P, C, Fp, Fa, T = 2, 2, 2, 3, 4, 10
    M = np.zeros((E, P, Fp, Fa), dtype=np.complex128)
    amp = np.zeros((E, C, Fa, 2))
    phase = np.zeros((E, C, Fp), dtype=np.complex128)
    for kind in KINDS:                                            # a zero amplitude row: 0, not NaN
        got = finalize_pac(kind, M, amp, phase, [0, 1], [1, 1], T)
        assert got.shape == (E, P, Fp, Fa) and not np.any(got), kind
    # only the amplitude channel's sums matter: channel 0 zero, channel 1 not
    amp[:, 1] = [5., 4.]
    M[:, 0] = 3.                                                  # pair 0 = (0, 1): denominators 5 and sqrt(40)
    got = finalize_pac('mvl_norm', M, amp, phase, [0, 1], [1, 0], T)
    assert np.array_equal(got[:, 0], np.full((E, Fp, Fa), 3. / 5.)) and not np.any(got[:, 1])
    got = finalize_pac('direct_pac', M, amp, phase, [0, 1], [1, 0], T)
    assert np.allclose(got[:, 0], 3. / np.sqrt(40.)) and not np.any(got[:, 1])


def test_index_and_scale_checks():
    ip, ia = check_pac_indices(None, 4)
    assert ip.dtype == np.int32 and np.array_equal(ip, [0, 1, 2, 3]) and np.array_equal(ia, ip)
    ip, ia = check_pac_indices(([2, 0, 0], [0, 0, 3]), 4)
    assert np.array_equal(ip, [2, 0, 0]) and np.array_equal(ia, [0, 0, 3])
    with pytest.raises(ValueError, match='indices'):
        check_pac_indices(([0], [4]), 4)
    got = check_scales('phase', [3, 0, 3, 8], 9)
    assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, [3, 0, 3, 8])
    assert np.array_equal(check_scales('amp', range(4, 9), 9), [4, 5, 6, 7, 8])
    for bad in ([], None, [9], [-1, 2], [0.5], [[0, 1]], 3, 'ab'):
        with pytest.raises(ValueError, match='phase'):
            check_scales('phase', bad, 9)


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    freqs = [4., 7., 12., 40., 70.]
    w = nw.Morse(1000)
    ok = dict(phase=[0, 1], amp=[3, 4])
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.pac_batch(x, freqs, decim=decim, **ok)
    for out in ('cwt', 'coherence', 'wpli', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.pac_batch(x, freqs, out=out, **ok)
    with pytest.raises(ValueError, match='average'):
        w.pac_batch(x, freqs, out='pac_sum', average=True, **ok)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.pac_batch(bad, freqs, **ok)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.pac_batch(x, freqs, indices=idx, **ok)
    for bad in ([5], [-1], [0, 7], [], None, [1.5]):              # scale positions out of range, empty lists
        with pytest.raises(ValueError, match='phase'):
            w.pac_batch(x, freqs, phase=bad, amp=[3, 4])
        with pytest.raises(ValueError, match='amp'):
            w.pac_batch(x, freqs, phase=[0, 1], amp=bad)
    with pytest.raises(ValueError, match='phase'):                # the defaults are no lists
        w.pac_batch(x, freqs)
    for win in ((-1, 5), (6, 5), (0, 4097), (0.5, 3), (1,), 7):
        with pytest.raises(ValueError, match='window'):
            w.pac_batch(x, freqs, window=win, **ok)
    for kind in KINDS:                                            # an empty window has no finalised measure
        with pytest.raises(ValueError, match='at least 1'):
            w.pac_batch(x, freqs, out=kind, window=(8, 8), **ok)
        with pytest.raises(ValueError, match='at least 1'):
            w.pac_batch(x, freqs, out=kind, window=(1, 4), decim=4, **ok)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.pac(['a', 'b'], [4., 7.], [40., 70.], decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.pac(['a', 'b'], [4., 7.], [40., 70.], method='itc')
    with pytest.raises(ValueError, match='indices'):
        ew.pac(['a', 'b'], [4., 7.], [40., 70.], indices=([0], [2]))
    with pytest.raises(ValueError):
        ew.pac(['a', 'z'], [4., 7.], [40., 70.])                  # no such channel
    with pytest.raises(ValueError, match='phase'):
        ew.pac(['a', 'b'], [], [40., 70.])
    with pytest.raises(ValueError, match='amp'):
        ew.pac(['a', 'b'], [4., 7.], [])
    for padding in (2.048, 3., -0.1, float('nan')):
        with pytest.raises(ValueError, match='padding'):
            ew.pac(['a', 'b'], [4., 7.], [40., 70.], padding=padding)
    with pytest.raises(ValueError, match='average'):
        ew.pac(['a', 'b'], [4., 7.], [40., 70.], method='pac_sum', average=True)
    assert w._cache is None and not w._plans


def test_constants_and_exports():
    assert L.NW_REDUCE_PAC == 5
    assert {L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS, L.NW_REDUCE_CONN, L.NW_REDUCE_CONN_TIME,
            L.NW_REDUCE_PAC} == set(range(6))
    assert PAC_OUTS == {'pac_sum', 'mvl', 'mvl_norm', 'direct_pac', 'debiased_pac'}
    assert nw.finalize_pac is finalize_pac and 'finalize_pac' in nw.__all__
    assert hasattr(nw.Plan, 'execute_pac') and hasattr(nw.WaveletBase, 'pac_batch') and hasattr(nw.EpochsWavelet, 'pac')
    sig = {s[0]: s for s in L.SIGNATURES}
    assert 'nw_execute_pac' in sig and len(sig['nw_execute_pac'][2]) == 18
    with open(os.path.join(ROOT, 'include', 'ninwave.h')) as f:
        header = f.read()
    assert '#define NW_REDUCE_PAC      5' in header and 'int nw_execute_pac(' in header
    assert hasattr(L.lib(), 'nw_execute_pac')                     # the library exports it (host-only load)
