"""Time-lag surrogate statistics of the phase-amplitude coupling without a GPU: the surrogate kernels' geometry
(nw_shape.h, a stand-alone host program), the numpy finaliser engine.finalize_pac_surr against direct formulas for
every measure and statistic, the lag draw and the lag check, the argument checks of the three Python layers that
fire before any device work, and the new constants, exports and signature."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FakeEpochs

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd import engine
from ninwavelets_amd.engine import PAC_SURR_STATS, check_lags, draw_lags, finalize_pac, finalize_pac_surr

KINDS = ('mvl', 'mvl_norm', 'direct_pac', 'debiased_pac')
STATS = ('zscore', 'pvalue', 'surr_mean', 'surr_std', 'surr_max', 'surrogates')


def test_staging_layout_shift_and_cell_lanes_on_the_host(tmp_path):
    """tests/asan/pac_surr_shape.cpp (a stand-alone program over nw_shape.h) under -fsanitize=address,undefined:
    the staged planes tile the scratch, the staging launch writes every slot once, the circular shift is
    (j + l) mod T in two contiguous runs, and a wave's cells have one lane each."""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'pac_surr_shape')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'asan', 'pac_surr_shape.cpp'), '-o', exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def _sums(rng, E, C, F, T, fph, fam, ip, ia, lags, debiased):
    """The surrogate sums of random rows (E, C, F, T), formed directly: (M, amp, phase, stat, all, Mc_0, Mc_s)."""
    y = rng.standard_normal((E, C, F, T)) + 1j * rng.standard_normal((E, C, F, T))
    A = np.abs(y[:, :, fam])                                      # (E, C, Fa, T)
    u = y[:, :, fph] / np.abs(y[:, :, fph])                       # (E, C, Fp, T)
    Ms = np.stack([np.einsum('epit,epkt->epik', u[:, ip], np.roll(A, -l, axis=-1)[:, ia].astype(np.complex128))
                   for l in [0] + list(lags)], axis=-1)           # (E, P, Fp, Fa, 1 + S): A[(j + l) mod T] u[j]
    amp = np.stack([A.sum(-1), (A * A).sum(-1)], axis=-1)
    phase = u.sum(-1)
    D = phase[:, ip][:, :, :, None] * amp[:, ia][:, :, None, :, 0] / T if debiased else 0.
    Mc = Ms - np.asarray(D)[..., None]
    q = Mc.real ** 2 + Mc.imag ** 2
    qs = q[..., 1:]
    stat = np.stack([np.sqrt(qs).sum(-1), qs.sum(-1), (qs >= q[..., :1]).sum(-1).astype(np.float64),
                     qs.max(-1, initial=0.)], axis=-1)
    return Ms[..., 0], amp, phase, stat, np.ascontiguousarray(Ms[..., 1:]), Mc[..., 0], Mc[..., 1:]


def test_finalize_pac_surr_against_direct_formulas():
    rng = np.random.default_rng(12)
    E, C, F, T = 3, 3, 7, 50
    fph, fam = np.array([0, 1, 1]), np.array([2, 6, 3, 2])
    ip, ia = np.array([0, 2, 1, 1]), np.array([1, 0, 1, 2])
    lags = np.array([5, 17, 0, 49, 17, 30, 1, 12])
    S = len(lags)
    assert PAC_SURR_STATS == set(STATS) | {'surr_sum'}
    for kind in KINDS:
        M, amp, phase, stat, all_, Mc0, Mcs = _sums(rng, E, C, F, T, fph, fam, ip, ia, lags, kind == 'debiased_pac')
        # the measure of each surrogate, by finalize_pac's own denominators: a shift changes neither sum A nor sum A^2
        sA, sA2 = amp[:, ia][:, :, None, :, 0], amp[:, ia][:, :, None, :, 1]
        den = {'mvl': T, 'mvl_norm': sA, 'direct_pac': np.sqrt(T * sA2), 'debiased_pac': T}[kind] * np.ones(M.shape)
        obs = finalize_pac(kind, M, amp, phase, ip, ia, T)
        assert np.allclose(obs, np.abs(Mc0) / den, rtol=1e-12)
        vals = np.abs(Mcs) / den[..., None]                        # (E, P, Fp, Fa, S)
        want = {'zscore': (obs - vals.mean(-1)) / vals.std(-1), 'pvalue': (1 + (vals >= obs[..., None]).sum(-1)) / (1 + S),
                'surr_mean': vals.mean(-1), 'surr_std': vals.std(-1), 'surr_max': vals.max(-1), 'surrogates': vals}
        for sk, ref in want.items():
            got = finalize_pac_surr(kind, sk, M, amp, phase, stat, all_, ip, ia, T, S)
            assert got.shape == ref.shape and got.dtype == np.float64, (kind, sk)
            # (the sd is a difference of two sums: a few digits go)
            assert np.allclose(got, ref, rtol=1e-7 if sk in ('zscore', 'surr_std') else 1e-12, atol=1e-12), (kind, sk)
        # the statistics need no ``all``; the surrogates do
        assert finalize_pac_surr(kind, 'pvalue', M, amp, phase, stat, None, ip, ia, T, S).shape == M.shape
        with pytest.raises(ValueError, match='keep_all'):
            finalize_pac_surr(kind, 'surrogates', M, amp, phase, stat, None, ip, ia, T, S)
        got = finalize_pac_surr(kind, 'surr_sum', M, amp, phase, stat, all_, ip, ia, T, S)
        assert got[0] is M and got[1] is amp and got[2] is phase and got[3] is stat and got[4] is all_
        # empty epoch and pair axes keep their shapes
        for sk in STATS[:-1]:
            assert finalize_pac_surr(kind, sk, M[:0], amp[:0], phase[:0], stat[:0], None, ip, ia, T, S).shape == \
                (0, len(ip), len(fph), len(fam))
            assert finalize_pac_surr(kind, sk, M[:, :0], amp, phase, stat[:, :0], None, ip[:0], ia[:0], T, S).shape == \
                (E, 0, len(fph), len(fam))
    M, amp, phase, stat, all_, _, _ = _sums(rng, E, C, F, T, fph, fam, ip, ia, lags, False)
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_pac_surr('coherence', 'zscore', M, amp, phase, stat, all_, ip, ia, T, S)
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_pac_surr('pac_sum', 'zscore', M, amp, phase, stat, all_, ip, ia, T, S)
    with pytest.raises(ValueError, match='stat must be one of'):
        finalize_pac_surr('mvl', 'tscore', M, amp, phase, stat, all_, ip, ia, T, S)
    for kind in KINDS:
        for sk in STATS:
            for T0 in (0, -1):
                with pytest.raises(ValueError, match='at least 1 sample'):
                    finalize_pac_surr(kind, sk, M, amp, phase, stat, all_, ip, ia, T0, S)
            with pytest.raises(ValueError, match='at least'):
                finalize_pac_surr(kind, sk, M, amp, phase, stat, all_[..., :0], ip, ia, T, 0)
        for sk in ('zscore', 'surr_std'):
            with pytest.raises(ValueError, match='at least 2 surrogates'):
                finalize_pac_surr(kind, sk, M, amp, phase, stat, all_[..., :1], ip, ia, T, 1)
        for sk in ('pvalue', 'surr_mean', 'surr_max'):             # one surrogate is enough for these
            assert finalize_pac_surr(kind, sk, M, amp, phase, stat, None, ip, ia, T, 1).shape == M.shape
    assert finalize_pac_surr('pac_sum', 'surr_sum', M, amp, phase, stat, None, ip, ia, 0, 0)[3] is stat


def test_finalize_pac_surr_flat_surrogates_and_zero_denominators():
    """sd = 0 gives z = 0, not a division by zero; a zero amplitude row gives 0 in the measure's units."""
    E, P, C, Fp, Fa, T, S = 2, 2, 2, 3, 4, 10, 5
    M = np.full((E, P, Fp, Fa), 3. + 4.j)
    amp = np.zeros((E, C, Fa, 2))
    amp[:, 1] = [5., 4.]
    phase = np.zeros((E, C, Fp), dtype=np.complex128)
    stat = np.empty((E, P, Fp, Fa, 4))
    stat[...] = [S * 2., S * 4., 0., 4.]                          # every surrogate has h = 2: mean 2, sd 0
    ip, ia = [0, 1], [1, 0]
    for kind in KINDS:
        with np.errstate(all='raise'):
            z = finalize_pac_surr(kind, 'zscore', M, amp, phase, stat, None, ip, ia, T, S)
            sd = finalize_pac_surr(kind, 'surr_std', M, amp, phase, stat, None, ip, ia, T, S)
        assert not np.any(z) and not np.any(sd), kind
        assert np.array_equal(finalize_pac_surr(kind, 'pvalue', M, amp, phase, stat, None, ip, ia, T, S),
                              np.full(M.shape, 1. / 6.))
    mean = finalize_pac_surr('mvl_norm', 'surr_mean', M, amp, phase, stat, None, ip, ia, T, S)
    assert np.array_equal(mean[:, 0], np.full((E, Fp, Fa), 2. / 5.)) and not np.any(mean[:, 1])     # channel 0: sum A = 0
    mx = finalize_pac_surr('direct_pac', 'surr_max', M, amp, phase, stat, None, ip, ia, T, S)
    assert np.allclose(mx[:, 0], 2. / np.sqrt(40.)) and not np.any(mx[:, 1])
    assert np.array_equal(finalize_pac_surr('mvl', 'surr_mean', M, amp, phase, stat, None, ip, ia, T, S),
                          np.full(M.shape, 0.2))
    # a slightly negative variance (rounding) is clipped: sd = 0, z = 0
    stat[..., 1] = S * 4. * (1 - 1e-15)
    assert not np.any(finalize_pac_surr('mvl', 'zscore', M, amp, phase, stat, None, ip, ia, T, S))
    # NaN sums (a zero phase sample) stay NaN
    stat[0, 0, 0, 0, :2] = np.nan
    z = finalize_pac_surr('mvl', 'zscore', M, amp, phase, stat, None, ip, ia, T, S)
    assert np.isnan(z[0, 0, 0, 0]) and np.count_nonzero(np.isnan(z)) == 1


def test_lag_draw_and_lag_check():
    for T, S, seed in ((964, 200, 3), (1024, 32, 0), (20, 7, 5), (2, 4, 1)):
        lo = max(1, T // 10)
        a, b = draw_lags(T, S, seed=seed), draw_lags(T, S, seed=seed)
        assert a.dtype == np.int64 and a.shape == (S,) and np.array_equal(a, b)
        assert np.array_equal(a, np.random.default_rng(seed).integers(lo, T - lo + 1, S))
        assert a.min() >= lo and a.max() <= T - lo
    assert not np.array_equal(draw_lags(964, 200, seed=3), draw_lags(964, 200, seed=4))
    a = draw_lags(964, 500, min_lag=400, seed=9)
    assert a.min() >= 400 and a.max() <= 564 and {400, 564} <= set(a.tolist())       # both ends are drawn
    assert set(draw_lags(10, 50, min_lag=5, seed=1).tolist()) == {5}
    for T, lo in ((1, None), (0, None), (9, 5), (964, 483)):
        with pytest.raises(ValueError, match='min_lag'):
            draw_lags(T, 10, min_lag=lo)
    for lo in (0, -3):
        with pytest.raises(ValueError, match='min_lag'):
            draw_lags(964, 10, min_lag=lo)
    for S in (0, -1, L.NW_PAC_MAX_LAGS + 1, 2.5, None):
        with pytest.raises(ValueError, match='n_surrogates'):
            draw_lags(964, S)
    assert draw_lags(964, L.NW_PAC_MAX_LAGS, seed=0).size == L.NW_PAC_MAX_LAGS
    got = check_lags([3, 0, 3, 963], 964)
    assert got.dtype == np.int64 and got.flags.c_contiguous and np.array_equal(got, [3, 0, 3, 963])
    assert check_lags([], 964).shape == (0,) and check_lags(np.arange(5, dtype=np.int32), 5).dtype == np.int64
    assert check_lags([], 0).shape == (0,)
    for bad in ([964], [-1, 2], [0.5], [[0, 1]], 3, 'ab', None, np.zeros(L.NW_PAC_MAX_LAGS + 1, dtype=np.int64)):
        with pytest.raises(ValueError, match='lags'):
            check_lags(bad, 964)
    with pytest.raises(ValueError, match='lags'):
        check_lags([0], 0)                                        # an empty window has no lag


def test_bad_arguments_are_value_errors_before_any_device_work(monkeypatch):
    """No device is touched: the loader is replaced by one that fails, and the checks come before the cache build
    and the plan."""
    def no_device(*a, **k):
        raise AssertionError('the library was loaded: device work before the argument checks')
    x = np.zeros((3, 4, 4096))
    freqs = [4., 7., 12., 40., 70.]
    w = nw.Morse(1000)
    ok = dict(phase=[0, 1], amp=[3, 4])
    monkeypatch.setattr(L, 'lib', no_device)
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.pac_surrogates_batch(x, freqs, decim=decim, **ok)
    for out in ('cwt', 'coherence', 'pac_sum', 'mi', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.pac_surrogates_batch(x, freqs, out=out, **ok)
    for stat in ('tscore', 'mean', None):
        with pytest.raises(ValueError, match='stat must be one of'):
            w.pac_surrogates_batch(x, freqs, stat=stat, **ok)
    for stat in ('pvalue', 'surr_max', 'surrogates', 'surr_sum'):
        with pytest.raises(ValueError, match='average'):
            w.pac_surrogates_batch(x, freqs, stat=stat, average=True, **ok)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.pac_surrogates_batch(bad, freqs, **ok)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.pac_surrogates_batch(x, freqs, indices=idx, **ok)
    for bad in ([5], [-1], [0, 7], [], None, [1.5]):              # scale positions out of range, empty lists
        with pytest.raises(ValueError, match='phase'):
            w.pac_surrogates_batch(x, freqs, phase=bad, amp=[3, 4])
        with pytest.raises(ValueError, match='amp'):
            w.pac_surrogates_batch(x, freqs, phase=[0, 1], amp=bad)
    for win in ((-1, 5), (6, 5), (0, 4097), (0.5, 3), (1,), 7):
        with pytest.raises(ValueError, match='window'):
            w.pac_surrogates_batch(x, freqs, window=win, **ok)
    for stat in sorted(PAC_SURR_STATS):                           # an empty window has no surrogate
        with pytest.raises(ValueError, match='at least 1 sample'):
            w.pac_surrogates_batch(x, freqs, stat=stat, window=(8, 8), **ok)
        with pytest.raises(ValueError, match='at least 1 sample'):
            w.pac_surrogates_batch(x, freqs, stat=stat, window=(1, 4), decim=4, **ok)
    # the lags: explicit lists in [0, T) of the window's decimated samples, at most NW_PAC_MAX_LAGS
    for bad in ([100], [-1], [0.5], [[1, 2]], 'ab', np.zeros(L.NW_PAC_MAX_LAGS + 1, dtype=np.int64)):
        with pytest.raises(ValueError, match='lags'):
            w.pac_surrogates_batch(x, freqs, lags=bad, window=(0, 100), **ok)
    with pytest.raises(ValueError, match='lags'):
        w.pac_surrogates_batch(x, freqs, lags=[25], window=(0, 100), decim=4, **ok)     # T = 25
    for stat in ('zscore', 'surr_std'):
        with pytest.raises(ValueError, match='at least 2 surrogates'):
            w.pac_surrogates_batch(x, freqs, stat=stat, lags=[7], **ok)
        with pytest.raises(ValueError, match='at least 2 surrogates'):
            w.pac_surrogates_batch(x, freqs, stat=stat, n_surrogates=1, **ok)
    for stat in ('pvalue', 'surr_mean', 'surr_max', 'surrogates'):
        with pytest.raises(ValueError, match='at least 1 surrogate'):
            w.pac_surrogates_batch(x, freqs, stat=stat, lags=[], **ok)
    # the draw
    for S in (0, -1, L.NW_PAC_MAX_LAGS + 1, 1.5):
        with pytest.raises(ValueError, match='n_surrogates'):
            w.pac_surrogates_batch(x, freqs, n_surrogates=S, **ok)
    for lo in (0, -1, 2049, 1.5):
        with pytest.raises(ValueError, match='min_lag'):
            w.pac_surrogates_batch(x, freqs, min_lag=lo, **ok)
    with pytest.raises(ValueError, match='min_lag'):
        w.pac_surrogates_batch(x, freqs, window=(5, 6), **ok)      # T = 1 < 2 min_lag
    with pytest.raises(ValueError, match='min_lag'):
        w.pac_surrogates_batch(x, freqs, min_lag=13, window=(0, 100), decim=4, **ok)     # T = 25 < 26
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], method='pac_sum')
    with pytest.raises(ValueError, match='stat must be one of'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], stat='itc')
    with pytest.raises(ValueError, match='indices'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], indices=([0], [2]))
    with pytest.raises(ValueError):
        ew.pac_surrogates(['a', 'z'], [4., 7.], [40., 70.])        # no such channel
    with pytest.raises(ValueError, match='phase'):
        ew.pac_surrogates(['a', 'b'], [], [40., 70.])
    with pytest.raises(ValueError, match='amp'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [])
    for padding in (2.048, 3., -0.1, float('nan')):
        with pytest.raises(ValueError, match='padding'):
            ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], padding=padding)
    with pytest.raises(ValueError, match='lags'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], lags=[4000], padding=0.1)      # T = 3896
    with pytest.raises(ValueError, match='average'):
        ew.pac_surrogates(['a', 'b'], [4., 7.], [40., 70.], stat='pvalue', average=True)
    assert w._cache is None and not w._plans


class _NoPlan:
    """What Plan.execute_pac_surr reads of a plan before its first device call."""
    nfreq, n, n_out, dtype, device = 9, 1024, 1024, np.dtype('float64'), 0
    _window = engine.Plan._window
    _epoch_input = engine.Plan._epoch_input
    _outputs = engine.Plan._outputs

    def _epoch_execute(self, *a, **k):
        raise AssertionError('the call reached the device')


def test_plan_layer_checks_come_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the library was loaded: device work before the argument checks')
    monkeypatch.setattr(L, 'lib', no_device)
    p = _NoPlan()
    call = engine.Plan.execute_pac_surr
    x = np.zeros((2, 3, 1024))
    ok = dict(phase=[0, 1], amp=[4, 5])
    for bad in ([964], [-1], [0.5], [[0, 1]], 3, None, np.zeros(L.NW_PAC_MAX_LAGS + 1, dtype=np.int64)):
        with pytest.raises(ValueError, match='lags'):
            call(p, x, bad, window=(37, 1001), **ok)
    with pytest.raises(ValueError, match='lags'):
        call(p, x, [241], window=(37, 1001), step=4, **ok)        # T = 241
    with pytest.raises(ValueError, match='lags'):
        call(p, x, [0], window=(5, 5), **ok)
    for centre in ('debiased_pac', 'mvl', None, 1):
        with pytest.raises(ValueError, match='centre'):
            call(p, x, [1, 2], centre=centre, **ok)
    with pytest.raises(ValueError, match='window'):
        call(p, x, [1], window=(0, 1025), **ok)
    with pytest.raises(ValueError, match='step'):
        call(p, x, [1], step=0, **ok)
    with pytest.raises(ValueError, match='phase'):
        call(p, x, [1], phase=[9], amp=[4])
    with pytest.raises(ValueError, match='amp'):
        call(p, x, [1], phase=[0], amp=[])
    with pytest.raises(ValueError, match='indices'):
        call(p, x, [1], indices=([0], [3]), **ok)
    with pytest.raises(ValueError, match='epochs, channels'):
        call(p, x.reshape(6, 1024), [1], **ok)
    with pytest.raises(ValueError, match='signal length'):
        call(p, np.zeros((2, 3, 1000)), [1], **ok)
    with pytest.raises(ValueError, match='M, amp, phase, stat'):
        call(p, x, [1, 2], out=(None, None, None), **ok)          # four buffers, five with keep_all
    with pytest.raises(ValueError, match='M, amp, phase, stat'):
        call(p, x, [1, 2], keep_all=True, out=(None, None, None, None), **ok)
    with pytest.raises(ValueError, match='right dtype and size'):
        call(p, x, [1, 2], out=(None, None, None, np.empty((2, 3, 2, 2, 3))), **ok)
    with pytest.raises(ValueError, match='right dtype and size'):
        call(p, x, [1, 2], keep_all=True, out=(None, None, None, None, np.empty((2, 3, 2, 2, 3), dtype=np.complex128)), **ok)
    with pytest.raises(AssertionError, match='the library was loaded'):   # ... and good arguments go on to the device
        call(p, x, [1, 2], **ok)


def test_constants_and_exports():
    assert L.NW_REDUCE_PAC_SURR == 9 and L.NW_PAC_MAX_LAGS == 4096
    assert (L.NW_PAC_SURR_PLAIN, L.NW_PAC_SURR_DEBIASED) == (0, 1)
    assert {L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS, L.NW_REDUCE_CONN, L.NW_REDUCE_CONN_TIME,
            L.NW_REDUCE_PAC, L.NW_REDUCE_ENV, L.NW_REDUCE_PAC_BINS, L.NW_REDUCE_ERPAC, L.NW_REDUCE_PAC_SURR} == set(range(10))
    assert engine.PAC_SURR_CENTRES == {'plain': 0, 'debiased': 1}
    assert PAC_SURR_STATS == {'surr_sum', 'zscore', 'pvalue', 'surr_mean', 'surr_std', 'surr_max', 'surrogates'}
    assert nw.finalize_pac_surr is finalize_pac_surr and 'finalize_pac_surr' in nw.__all__
    assert hasattr(nw.Plan, 'execute_pac_surr') and hasattr(nw.WaveletBase, 'pac_surrogates_batch')
    assert hasattr(nw.EpochsWavelet, 'pac_surrogates')
    par = inspect.signature(nw.WaveletBase.pac_surrogates_batch).parameters
    assert (par['out'].default, par['stat'].default, par['n_surrogates'].default) == ('direct_pac', 'zscore', 200)
    assert par['lags'].default is None and par['min_lag'].default is None and par['seed'].default is None
    par = inspect.signature(nw.Plan.execute_pac_surr).parameters
    assert par['centre'].default == 'plain' and par['keep_all'].default is False
    sig = {s[0]: s for s in L.SIGNATURES}
    assert 'nw_execute_pac_surr' in sig and len(sig['nw_execute_pac_surr'][2]) == 23
    with open(os.path.join(ROOT, 'include', 'ninwave.h')) as f:
        header = f.read()
    assert '#define NW_REDUCE_PAC_SURR 9' in header and 'int nw_execute_pac_surr(' in header
    assert '#define NW_PAC_MAX_LAGS 4096' in header
    assert '#define NW_PAC_SURR_PLAIN 0' in header and '#define NW_PAC_SURR_DEBIASED 1' in header
    assert hasattr(L.lib(), 'nw_execute_pac_surr')                # the library exports it (host-only load)
