"""Envelope correlation without a GPU: the numpy finaliser engine.finalize_env against a direct restatement
of mne-connectivity's envelope_correlation procedure on the oracle's rows (C1), its conventions (C2), the
argument checks of the plan-free layers that fire before any device work, the new constants, exports and
signature, and a device-only compile of nw_env.hip's diagnostic switches.  (nw_shape.h gained no host code: the kernel reuses the pair tiles and the block map of
nw_execute_conn_time, which tests/asan/conn_time_shape.cpp covers.)"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FREQS, FakeEpochs
from epoch_cases import lagged_rows as oracle_rows

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import ENV_KINDS, ENV_OUTS, all_pairs, finalize_env

MEASURES = ('aec', 'aec_directed', 'aec_orth', 'aec_orth_signed')


def mne_envelope_correlation(data, orthogonalize, absolute=True):
    """mne-connectivity's envelope_correlation for one epoch of analytic signals ``data`` (C, T), restated:
    magnitudes with their means subtracted and their norms (a zero norm -> 1); per seed row i every row k's
    |Im(y_i conj(y_k) / |y_k|)| (i orthogonalised against k; the self entry zeroed), its mean subtracted, its
    norm (zero -> 1); corr[i, k] = the dot product over both norms; then |.| and (corr + corr.T) / 2.
    orthogonalize=False: plain correlations of the magnitudes."""
    mag = np.abs(data)
    conj_scaled = data.conj() / mag
    mag_nomean = mag - mag.mean(axis=-1, keepdims=True)
    mag_std = np.linalg.norm(mag_nomean, axis=-1)
    mag_std[mag_std == 0] = 1
    C = len(data)
    corr = np.empty((C, C))
    for i, row in enumerate(data):
        if not orthogonalize:
            orth, orth_std = mag_nomean[i], mag_std[i]
        else:
            orth = np.abs((row * conj_scaled).imag)
            orth[i] = 0.
            orth = orth - orth.mean(axis=-1, keepdims=True)
            orth_std = np.linalg.norm(orth, axis=-1)
            orth_std[orth_std == 0] = 1
        corr[i] = np.sum(orth * mag_nomean, axis=1) / mag_std / orth_std
    if not orthogonalize:
        return corr
    directed = corr.copy()
    if absolute:
        corr = np.abs(corr)
    return (corr.T + corr) / 2, directed


def direct_sums(yw, ia, ib):
    """(plain (E, P, F), orth (E, P, F, 6), chan (E, C, F, 2)) of rows yw (E, C, F, T) with numpy's sums."""
    A = np.abs(yw)
    u = yw / A
    a, b = u[:, ia], u[:, ib]
    q = np.abs(a.imag * b.real - a.real * b.imag)
    Aa, Ab = A[:, ia], A[:, ib]
    uu, vv = Aa * q, Ab * q
    orth = np.stack([uu.sum(-1), (uu * uu).sum(-1), (uu * Ab).sum(-1), vv.sum(-1), (vv * vv).sum(-1), (vv * Aa).sum(-1)],
                    axis=-1)
    chan = np.stack([A.sum(-1), (yw.real ** 2 + yw.imag ** 2).sum(-1)], axis=-1)
    return (Aa * Ab).sum(-1), orth, chan


@pytest.mark.parametrize('win', [(0, 1024), (37, 1001)], ids=['full', 'inner'])
def test_finalize_env_against_the_mne_procedure(win):
    """C1: every finalised kind within 1e-11 of the mean-subtracting procedure (the sum form loses about three
    digits: the smallest var / sum x^2 of these inputs is 1.2e-3)."""
    n, E, C = 1024, 3, 5
    _, y = oracle_rows(n, E, C, 'float64', FREQS)
    yw = y[..., win[0]:win[1]]
    T = yw.shape[-1]
    # every ordered pair and the self pairs
    ia, ib = (g.ravel() for g in np.meshgrid(np.arange(C), np.arange(C), indexing='ij'))
    plain, orth, chan = direct_sums(yw, ia, ib)
    F = len(FREQS)
    want = {k: np.empty((E, C, C, F) + ((2,) if k == 'aec_directed' else ())) for k in MEASURES}
    for e in range(E):
        for f in range(F):
            data = yw[e, :, f]
            want['aec'][e, :, :, f] = mne_envelope_correlation(data, False)
            want['aec_orth'][e, :, :, f], d = mne_envelope_correlation(data, True)
            want['aec_orth_signed'][e, :, :, f], _ = mne_envelope_correlation(data, True, absolute=False)
            want['aec_directed'][e, :, :, f, 0], want['aec_directed'][e, :, :, f, 1] = d, d.T
    for kind in MEASURES:
        got = finalize_env(kind, plain if kind == 'aec' else orth, chan, ia, ib, T)
        ref = want[kind].reshape((E, C * C) + want[kind].shape[3:])
        assert got.shape == ref.shape and got.dtype == np.float64, kind
        d = np.abs(got - ref).max()
        print(f'{win} {kind}: {d:.2e}')
        assert d <= 1e-11, (kind, d)
    own = ia == ib
    for kind in MEASURES[1:]:                                     # mne's diagonal: exactly 0
        assert not np.any(finalize_env(kind, orth, chan, ia, ib, T)[:, own]), kind
    aec = finalize_env('aec', plain, chan, ia, ib, T)
    assert np.abs(aec[:, own] - 1).max() <= 1e-11 and np.abs(aec).max() <= 1 + 1e-11


def test_finalize_env_conventions():
    """C2."""
    rng = np.random.default_rng(5)
    E, C, F, T = 2, 3, 4, 40
    ia, ib = np.array([0, 1, 2, 1]), np.array([1, 2, 2, 0])
    P = len(ia)
    y = rng.standard_normal((E, C, F, T)) + 1j * rng.standard_normal((E, C, F, T))
    y[:, 2] = 3. * np.exp(1j * rng.uniform(0, 6, (E, F, T)))     # channel 2: a constant envelope
    plain, orth, chan = direct_sums(y, ia, ib)
    chan[:, 2, :, 1] = chan[:, 2, :, 0] ** 2 / T                   # its variance: exactly <= 0
    # zero variance gives 0, not NaN or inf
    aec = finalize_env('aec', plain, chan, ia, ib, T)
    assert not np.any(aec[:, 1]) and not np.any(aec[:, 2]) and np.all(np.isfinite(aec)) and np.all(aec[:, 0] != 0)
    d = finalize_env('aec_directed', orth, chan, ia, ib, T)
    assert not np.any(d[:, 1, :, 0]) and np.all(d[:, 1, :, 1] != 0)       # r(u, A_2) = 0; r(v, A_1) is not
    zero = finalize_env('aec_orth', np.zeros_like(orth), np.zeros_like(chan), ia, ib, T)
    assert not np.any(zero) and zero.shape == (E, P, F)
    # a self pair gives exactly 0 whatever the sums hold
    junk = rng.standard_normal(orth.shape) + 5.
    for kind in MEASURES[1:]:
        assert not np.any(finalize_env(kind, junk, np.abs(chan) + 1., ia, ib, T)[:, 2]), kind
    # NaN sums (a sample with |y| = 0) stay NaN
    bad = orth.copy()
    bad[0, 0, 1] = np.nan
    got = finalize_env('aec_orth', bad, chan, ia, ib, T)
    assert np.isnan(got[0, 0, 1]) and np.isnan(got).sum() == 1
    # the relations between the kinds
    d = finalize_env('aec_directed', orth, chan, ia, ib, T)
    assert np.array_equal(finalize_env('aec_orth', orth, chan, ia, ib, T), (np.abs(d[..., 0]) + np.abs(d[..., 1])) / 2)
    assert np.array_equal(finalize_env('aec_orth_signed', orth, chan, ia, ib, T), (d[..., 0] + d[..., 1]) / 2)
    # swapping (a, b) swaps the directions: pair 3 = (1, 0) against pair 0 = (0, 1)
    assert np.allclose(d[:, 3, :, 0], d[:, 0, :, 1], rtol=0, atol=1e-13) and np.allclose(d[:, 3, :, 1], d[:, 0, :, 0],
                                                                                         rtol=0, atol=1e-13)
    # shapes and dtypes
    assert d.shape == (E, P, F, 2) and d.dtype == np.float64 and aec.shape == (E, P, F) and aec.dtype == np.float64
    for kind in MEASURES:
        src = plain if kind == 'aec' else orth
        tail = (2,) if kind == 'aec_directed' else ()
        assert finalize_env(kind, src[:0], chan[:0], ia, ib, T).shape == (0, P, F) + tail
        assert finalize_env(kind, src[:, :0], chan, ia[:0], ib[:0], T).shape == (E, 0, F) + tail
        assert finalize_env(kind, src.astype(np.float32), chan, ia, ib, T).dtype == np.float64
    # the sums pass through unchanged, whatever T
    for kind, src in (('env_sum', plain), ('env_orth_sum', orth)):
        got = finalize_env(kind, src, chan, ia, ib, 0)
        assert got[0] is src and got[1] is chan
    # T < 2 and unknown kinds raise; so do sums of the wrong mode
    for kind in MEASURES:
        for T0 in (1, 0, -3):
            with pytest.raises(ValueError, match='at least 2'):
                finalize_env(kind, plain if kind == 'aec' else orth, chan, ia, ib, T0)
    for kind in ('coherence', 'wpli', 'pac_sum', 'aec_log', None):
        with pytest.raises(ValueError, match='out must be one of'):
            finalize_env(kind, orth, chan, ia, ib, T)
    with pytest.raises(ValueError, match='pair sums'):
        finalize_env('aec', orth, chan, ia, ib, T)
    with pytest.raises(ValueError, match='pair sums'):
        finalize_env('aec_orth', plain, chan, ia, ib, T)
    with pytest.raises(ValueError, match='chan'):
        finalize_env('aec', plain, chan[..., 0], ia, ib, T)


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not available')
def test_diagnostic_switches_compile(tmp_path):
    """nw_env.hip's two ablation switches (tools/env_rate.py (d)) still build: a device-only compile, nothing runs."""
    out = str(tmp_path / 'nw_env.co')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++20', '--cuda-device-only',
                        '-DNW_ABL_ENV_NODIV', '-DNW_ABL_ENV_NOLOAD', '-c',
                        os.path.join(ROOT, 'ninwavelets_amd', 'csrc', 'nw_env.hip'), '-o', out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(out) > 0


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    freqs = [4., 7., 12., 40., 70.]
    w = nw.Morse(1000)
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.envelope_correlation_batch(x, freqs, decim=decim)
    for out in ('cwt', 'coherence', 'wpli', 'pac_sum', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.envelope_correlation_batch(x, freqs, out=out)
    for out in ('env_sum', 'env_orth_sum'):
        with pytest.raises(ValueError, match='average'):
            w.envelope_correlation_batch(x, freqs, out=out, average=True)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.envelope_correlation_batch(bad, freqs)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9]), 3):
        with pytest.raises(ValueError, match='indices'):
            w.envelope_correlation_batch(x, freqs, indices=idx)
    for win in ((-1, 5), (6, 5), (0, 4097), (0.5, 3), (1,), 7):
        with pytest.raises(ValueError, match='window'):
            w.envelope_correlation_batch(x, freqs, window=win)
    for kind in MEASURES:                                         # fewer than two samples: no correlation
        with pytest.raises(ValueError, match='at least 2'):
            w.envelope_correlation_batch(x, freqs, out=kind, window=(8, 9))
        with pytest.raises(ValueError, match='at least 2'):
            w.envelope_correlation_batch(x, freqs, out=kind, window=(1, 8), decim=4)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.envelope_correlation(['a', 'b'], [4., 7.], decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.envelope_correlation(['a', 'b'], [4., 7.], method='itc')
    with pytest.raises(ValueError, match='indices'):
        ew.envelope_correlation(['a', 'b'], [4., 7.], indices=([0], [2]))
    with pytest.raises(ValueError):
        ew.envelope_correlation(['a', 'z'], [4., 7.])             # no such channel
    for padding in (2.048, 3., -0.1, float('nan')):
        with pytest.raises(ValueError, match='padding'):
            ew.envelope_correlation(['a', 'b'], [4., 7.], padding=padding)
    with pytest.raises(ValueError, match='average'):
        ew.envelope_correlation(['a', 'b'], [4., 7.], method='env_sum', average=True)
    assert w._cache is None and not w._plans


def test_constants_and_exports():
    assert L.NW_REDUCE_ENV == 6 and (L.NW_ENV_PLAIN, L.NW_ENV_ORTH) == (0, 1)
    assert {L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS, L.NW_REDUCE_CONN, L.NW_REDUCE_CONN_TIME,
            L.NW_REDUCE_PAC, L.NW_REDUCE_ENV} == set(range(7))
    assert ENV_KINDS == {'env_sum': L.NW_ENV_PLAIN, 'env_orth_sum': L.NW_ENV_ORTH}
    assert set(ENV_OUTS) == set(ENV_KINDS) | set(MEASURES) and set(ENV_OUTS.values()) == set(ENV_KINDS)
    assert ENV_OUTS['aec'] == 'env_sum' and all(ENV_OUTS[k] == 'env_orth_sum' for k in MEASURES[1:])
    assert nw.finalize_env is finalize_env and 'finalize_env' in nw.__all__
    assert hasattr(nw.Plan, 'execute_env_time') and hasattr(nw.WaveletBase, 'envelope_correlation_batch')
    assert hasattr(nw.EpochsWavelet, 'envelope_correlation')
    sig = {s[0]: s for s in L.SIGNATURES}
    assert 'nw_execute_env_time' in sig and sig['nw_execute_env_time'][2] == sig['nw_execute_conn_time'][2]
    with open(os.path.join(ROOT, 'include', 'ninwave.h')) as f:
        header = f.read()
    assert '#define NW_REDUCE_ENV      6' in header and 'int nw_execute_env_time(' in header
    assert '#define NW_ENV_PLAIN 0' in header and '#define NW_ENV_ORTH  1' in header
    assert hasattr(L.lib(), 'nw_execute_env_time')                # the library exports it (host-only load)
    ia, ib = all_pairs(4)
    assert len(ia) == 6
