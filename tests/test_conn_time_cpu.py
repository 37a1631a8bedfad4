"""Over-time connectivity without a GPU: the window's sample count (nw_conn_time_count), the numpy
finaliser engine.finalize_conn_time against direct formulas for every kind, the window arithmetic of
WaveletBase.connectivity_time_batch (engine.time_window, a pure function), the kernel's block map and window
geometry (nw_shape.h, a stand-alone host program), the argument checks of the
batch and class calls that fire before any device work, and the new constant of nw_stats.reduce_path."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FakeEpochs

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import CONN_OUTS, LAG_OUTS, finalize_conn_time, time_window


def test_window_sample_count():
    n = 1024
    for step in (1, 4):
        for t0, t1 in ((0, n), (0, 1), (5, 6), (37, 1001), (3, 1022), (0, 0), (500, 500), (n, n), (n - 1, n)):
            want = len(range(t0, t1, step))
            assert L.conn_time_count(n, t0, t1, step) == want, (t0, t1, step)
    assert L.conn_time_count(n, 37, 1001, 1) == 964 and L.conn_time_count(n, 37, 1001, 4) == 241
    assert L.conn_time_count(n, 0, 1, 4) == 1 and L.conn_time_count(n, 0, 5, 4) == 2
    for t0, t1, step in ((-1, 5, 1), (6, 5, 1), (0, n + 1, 1), (n + 1, n + 1, 1), (0, 5, 0), (0, 5, -4)):
        with pytest.raises(ValueError, match='nw_conn_time_count'):
            L.conn_time_count(n, t0, t1, step)
    assert L.lib().nw_conn_time_count(n, 0, 5, 1, None) == L.NW_E_INVALID
    c = ctypes.c_int64(-7)
    assert L.lib().nw_conn_time_count(0, 0, 0, 1, ctypes.byref(c)) == 0 and c.value == 0


def test_block_map_and_window_geometry_on_the_host(tmp_path):
    """tests/asan/conn_time_shape.cpp (a stand-alone program over nw_shape.h) under
    -fsanitize=address,undefined: one block per (epoch, scale, pair tile) in both block orders, the
    window's sample count and the lane of a sample."""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'conn_time_shape')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'asan', 'conn_time_shape.cpp'), '-o', exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def _sums(rng, E, C, F, T):
    """Over-time sums of random rows (E, C, F, T) for the pairs below, formed directly."""
    y = rng.standard_normal((E, C, F, T)) + 1j * rng.standard_normal((E, C, F, T))
    ia, ib = np.array([0, 2, 1, 1]), np.array([1, 0, 1, 2])         # (1, 1): the self pair
    a, b = y[:, ia], y[:, ib]
    S = np.sum(a * np.conj(b), axis=-1)
    power = np.sum(np.abs(y) ** 2, axis=-1)
    phi = np.sum(a / np.abs(a) * np.conj(b / np.abs(b)), axis=-1)
    m = (a * np.conj(b)).imag
    lag = np.stack([m.sum(-1), np.abs(m).sum(-1), (m * m).sum(-1), np.sign(m).sum(-1)], axis=-1)
    return y, ia, ib, S, power, phi, lag


def test_finalize_conn_time_against_direct_formulas():
    rng = np.random.default_rng(7)
    E, C, F, T = 3, 3, 4, 50
    y, ia, ib, S, power, phi, lag = _sums(rng, E, C, F, T)
    # the self pair's S is its power exactly, as the device forms it
    S[:, 2] = power[:, 1]
    paa, pbb = power[:, ia], power[:, ib]
    l0, l1, l2, l3 = (lag[..., k] for k in range(4))
    r, i = phi.real / T, np.abs(phi.imag) / T
    with np.errstate(divide='ignore', invalid='ignore'):      # the self pair's 0 / 0, not compared
        want = {'csd': S / T, 'coherency': S / np.sqrt(paa * pbb), 'coherence': np.abs(S) / np.sqrt(paa * pbb),
                'imcoh': S.imag / np.sqrt(paa * pbb), 'plv': np.abs(phi) / T,
                'pli': np.abs(l3) / T, 'dpli': 0.5 + 0.5 * l3 / T,
                'pli2_unbiased': (T * (np.abs(l3) / T) ** 2 - 1) / (T - 1), 'wpli': np.abs(l0) / l1,
                'wpli2_debiased': (l0 ** 2 - l2) / (l1 ** 2 - l2), 'ciplv': i / np.sqrt(1 - r * r),
                'ppc': (np.abs(phi) ** 2 - T) / (T * (T - 1))}
    assert set(want) | {'cross_sum', 'plv_sum', 'lag_sum'} == set(CONN_OUTS) | set(LAG_OUTS)
    for kind, ref in want.items():
        src = {'cross_sum': S, 'plv_sum': phi, 'lag_sum': lag}[CONN_OUTS[kind] if kind in CONN_OUTS else LAG_OUTS[kind]]
        got = finalize_conn_time(kind, src, power if src is S else None, ia, ib, T)
        assert got.shape == (E, len(ia), F), kind
        assert got.dtype == (np.complex128 if kind in ('csd', 'coherency') else np.float64), kind
        sel = [0, 1, 3] if kind in ('wpli', 'wpli2_debiased', 'ciplv') else slice(None)
        assert np.allclose(got[:, sel], ref[:, sel], rtol=1e-12, atol=1e-14), kind
    # the sums pass through
    got = finalize_conn_time('cross_sum', S, power, ia, ib, T)
    assert got[0] is S and got[1] is power
    assert finalize_conn_time('plv_sum', phi, None, ia, ib, T) is phi
    assert finalize_conn_time('lag_sum', lag, None, ia, ib, T) is lag
    # the self pair: coherence exactly 1, imcoh exactly 0
    assert np.array_equal(finalize_conn_time('coherence', S, power, ia, ib, T)[:, 2], np.ones((E, F)))
    assert not np.any(finalize_conn_time('imcoh', S, power, ia, ib, T)[:, 2])
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_conn_time('power_mean', S, power, ia, ib, T)
    for kind, src in (('pli2_unbiased', lag), ('ppc', phi)):
        with pytest.raises(ValueError, match='at least 2'):
            finalize_conn_time(kind, src, None, ia, ib, 1)
    # empty epoch and pair axes keep their shapes
    assert finalize_conn_time('coherence', S[:0], power[:0], ia, ib, T).shape == (0, len(ia), F)
    assert finalize_conn_time('wpli', lag[:, :0], None, ia[:0], ib[:0], T).shape == (E, 0, F)


def test_finalize_conn_time_zero_denominators():
    E, P, F, T = 2, 2, 3, 10
    lag = np.zeros((E, P, F, 4))
    # every m = 0: wpli and wpli2_debiased are 0, not NaN
    assert not np.any(finalize_conn_time('wpli', lag, None, [0, 0], [0, 1], T))
    assert not np.any(finalize_conn_time('wpli2_debiased', lag, None, [0, 0], [0, 1], T))
    assert np.array_equal(finalize_conn_time('dpli', lag, None, [0, 0], [0, 1], T), np.full((E, P, F), 0.5))
    # one sample m: L1^2 - L2 = 0 -> 0
    lag[..., 0], lag[..., 1], lag[..., 2], lag[..., 3] = -2., 2., 4., -1.
    assert not np.any(finalize_conn_time('wpli2_debiased', lag, None, [0, 0], [0, 1], T))
    assert np.array_equal(finalize_conn_time('wpli', lag, None, [0, 0], [0, 1], T), np.ones((E, P, F)))


@pytest.mark.parametrize('decim', [1, 4, 3])
def test_window_arithmetic(decim):
    """The samples summed are the decimated samples j * decim in [t0, t1), on either kind of plan."""
    n = 96
    for t0, t1 in ((0, n), (0, 1), (5, 6), (7, 90), (8, 88), (13, 13), (n, n), (n - 1, n), (1, 2), (94, 96)):
        want = [s for s in range(0, n, decim) if t0 <= s < t1]
        s0, s1, step, T = time_window(n, decim, (t0, t1), False)
        assert 0 <= s0 <= s1 <= n and step == decim and T == len(want), (t0, t1)
        assert list(range(s0, s1, step)) == want, (t0, t1)
        assert L.conn_time_count(n, s0, s1, step) == T
        if n % decim == 0:
            j0, j1, one, Td = time_window(n, decim, (t0, t1), True)
            assert one == 1 and 0 <= j0 <= j1 <= n // decim and Td == len(want), (t0, t1)
            assert [j * decim for j in range(j0, j1)] == want, (t0, t1)
    assert time_window(n, decim, None, False) == (0, n, decim, -(-n // decim))
    for bad in ((-1, 5), (6, 5), (0, n + 1), (0.5, 3), (1,), 3, 'ab', (1, 2, 3)):
        with pytest.raises(ValueError, match='window'):
            time_window(n, decim, bad, False)


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    freqs = [1., 2., 3.]
    w = nw.Morse(1000)
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.connectivity_time_batch(x, freqs, decim=decim)
    for out in ('cwt', 'power_mean', 'itc', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.connectivity_time_batch(x, freqs, out=out)
    for out in ('cross_sum', 'plv_sum', 'lag_sum'):
        with pytest.raises(ValueError, match='average'):
            w.connectivity_time_batch(x, freqs, out=out, average=True)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.connectivity_time_batch(bad, freqs)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.connectivity_time_batch(x, freqs, indices=idx)
    for win in ((-1, 5), (6, 5), (0, 4097), (0.5, 3), (1,), 7):
        with pytest.raises(ValueError, match='window'):
            w.connectivity_time_batch(x, freqs, window=win)
    for out in ('pli2_unbiased', 'ppc'):
        with pytest.raises(ValueError, match='at least 2'):
            w.connectivity_time_batch(x, freqs, out=out, window=(8, 9))
        with pytest.raises(ValueError, match='at least 2'):
            w.connectivity_time_batch(x, freqs, out=out, window=(1, 8), decim=4)      # only sample 4
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.connectivity_time(['a', 'b'], freqs, decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.connectivity_time(['a', 'b'], freqs, method='itc')
    with pytest.raises(ValueError, match='indices'):
        ew.connectivity_time(['a', 'b'], freqs, indices=([0], [2]))
    with pytest.raises(ValueError):
        ew.connectivity_time(['a', 'z'], freqs)                            # no such channel
    for padding in (2.048, 3., -0.1, float('nan')):                       # an empty window, a bad padding
        with pytest.raises(ValueError, match='padding'):
            ew.connectivity_time(['a', 'b'], freqs, padding=padding)
    with pytest.raises(ValueError, match='average'):
        ew.connectivity_time(['a', 'b'], freqs, method='cross_sum', average=True)
    # the older calls keep rejecting what they reject
    with pytest.raises(ValueError, match='out must be one of'):
        w.connectivity_batch(x, freqs, out='wpli')
    with pytest.raises(TypeError):
        w.connectivity_batch(x, freqs, window=(0, 5))
    assert w._cache is None and not w._plans


def test_constants_and_exports():
    assert L.NW_REDUCE_CONN_TIME == 4
    assert {L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS, L.NW_REDUCE_CONN, L.NW_REDUCE_CONN_TIME} == set(range(5))
    assert nw.finalize_conn_time is finalize_conn_time and 'finalize_conn_time' in nw.__all__
    assert hasattr(nw.Plan, 'execute_conn_time') and hasattr(nw.WaveletBase, 'connectivity_time_batch')
    assert hasattr(nw.EpochsWavelet, 'connectivity_time')
    names = [s[0] for s in L.SIGNATURES]
    assert 'nw_conn_time_count' in names and 'nw_execute_conn_time' in names
