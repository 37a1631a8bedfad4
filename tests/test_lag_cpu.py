"""Phase-lag connectivity without a GPU: the constants of the new sum kind, the numpy finaliser
engine.finalize_lag against the definitions written out from per-epoch terms, the argument checks of
WaveletBase.lag_batch / lag_connectivity_batch and EpochsWavelet.wpli / lag_connectivity (before any
device work) and the host-only predicate nw_pair_partials_supported (0 for NW_OUT_LAG_SUM)."""
import numpy as np
import pytest

from epoch_cases import FakeEpochs

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import LAG_KINDS, LAG_OUTS, finalize_lag

LAG_NAMES = ['pli', 'pli2_unbiased', 'dpli', 'wpli', 'wpli2_debiased']


def test_constants():
    assert L.NW_OUT_LAG_SUM == 9
    assert LAG_KINDS == {'lag_sum': L.NW_OUT_LAG_SUM}
    assert LAG_OUTS == {'lag_sum': 'lag_sum', 'pli': 'lag_sum', 'pli2_unbiased': 'lag_sum', 'dpli': 'lag_sum',
                        'wpli': 'lag_sum', 'wpli2_debiased': 'lag_sum', 'ciplv': 'plv_sum', 'ppc': 'plv_sum'}
    assert nw.finalize_lag is finalize_lag


def random_rows(seed, E=7, shape=(5, 33)):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((E,) + shape) + 1j * rng.standard_normal((E,) + shape)
    ya = 0.5 * common + rng.standard_normal((E,) + shape) + 1j * rng.standard_normal((E,) + shape)
    yb = 0.5 * common * np.exp(0.7j) + rng.standard_normal((E,) + shape) + 1j * rng.standard_normal((E,) + shape)
    return ya, yb


def lag_sums(ya, yb):
    # Im ya conj(yb) from rounded products, as the device forms it (numpy's complex product may
    # fuse one of them: a self pair would then leave the rounding error of the other)
    m = ya.imag * yb.real - ya.real * yb.imag
    return np.stack([m.sum(0), np.abs(m).sum(0), (m * m).sum(0), np.sign(m).sum(0)], axis=-1)


def plv_sum(ya, yb):
    return np.sum((ya / np.abs(ya)) * np.conj(yb / np.abs(yb)), axis=0)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_finalize_lag_matches_the_definitions(seed):
    E = 7
    ya, yb = random_rows(seed, E)
    m = (ya * np.conj(yb)).imag                               # (E, F, n): the per-epoch terms
    sums = lag_sums(ya, yb)
    phi = plv_sum(ya, yb)
    pli = np.abs(np.mean(np.sign(m), axis=0))
    plv = phi / E
    want = {'pli': pli,
            'dpli': np.mean(np.heaviside(m, 0.5), axis=0),
            'pli2_unbiased': (E * pli ** 2 - 1) / (E - 1),
            'wpli': np.abs(np.mean(m, axis=0)) / np.mean(np.abs(m), axis=0),
            'wpli2_debiased': (np.sum(m, 0) ** 2 - np.sum(m ** 2, 0)) / (np.sum(np.abs(m), 0) ** 2 - np.sum(m ** 2, 0)),
            'ciplv': np.abs(plv.imag) / np.sqrt(1 - plv.real ** 2),
            'ppc': (np.abs(phi) ** 2 - E) / (E * (E - 1))}
    # ppc written out as the mean of cos(dphi_j - dphi_k) over the epoch pairs j < k
    d = np.angle(ya * np.conj(yb))
    ppc_pairs = np.mean([np.cos(d[j] - d[k]) for j in range(E) for k in range(j + 1, E)], axis=0)
    assert np.max(np.abs(want['ppc'] - ppc_pairs)) <= 1e-14
    for kind, ref in want.items():
        got = finalize_lag(kind, phi if LAG_OUTS[kind] == 'plv_sum' else sums, E)
        assert got.shape == m.shape[1:] and got.dtype == np.float64, kind
        err = np.max(np.abs(got - ref))
        assert err <= 1e-14, (kind, err)
    assert finalize_lag('lag_sum', sums, E) is sums
    # any leading shape
    stacked = np.stack([sums, sums[::-1]])
    assert np.array_equal(finalize_lag('wpli', stacked, E)[1], finalize_lag('wpli', sums[::-1], E))
    assert np.all(finalize_lag('wpli', sums, E) <= 1) and np.all(finalize_lag('pli', sums, E) <= 1)


def test_zero_denominators_give_zero_and_a_self_pair_has_dpli_one_half():
    E = 5
    ya, _ = random_rows(4, E)
    own = lag_sums(ya, ya)                                    # a self pair: m_e = 0 exactly
    assert not np.any(own)
    zero = lag_sums(np.zeros_like(ya), np.zeros_like(ya))     # all-zero rows
    for sums in (own, zero):
        with np.errstate(all='raise'):                        # no 0 / 0 is ever formed
            assert np.array_equal(finalize_lag('wpli', sums, E), np.zeros(sums.shape[:-1]))
            assert np.array_equal(finalize_lag('wpli2_debiased', sums, E), np.zeros(sums.shape[:-1]))
            assert np.array_equal(finalize_lag('pli', sums, E), np.zeros(sums.shape[:-1]))
            assert np.array_equal(finalize_lag('dpli', sums, E), np.full(sums.shape[:-1], 0.5))
    # one epoch: |m| and m^2 cancel in the debiased denominator
    one = lag_sums(ya[:1], random_rows(5, 1)[1])
    assert np.array_equal(finalize_lag('wpli2_debiased', one, 1), np.zeros(one.shape[:-1]))
    assert np.array_equal(finalize_lag('wpli', one, 1), np.ones(one.shape[:-1]))
    # a NaN row poisons the measures
    bad = own.copy()
    bad[0, 0] = np.nan
    for kind in LAG_NAMES:
        out = finalize_lag(kind, bad, E)
        assert np.isnan(out[0, 0]) and not np.any(np.isnan(out[1:])), kind


def test_ciplv_at_unit_real_part():
    E = 4
    # the unit-phasor sums of perfectly locked pairs at lag 0 and pi: r = +-1 exactly
    phi = np.array([E + 0j, -E + 0j, E + 1e-3j, 0.5 * E + 0.25j * E, -E - 2e-3j])
    with np.errstate(all='raise'):
        got = finalize_lag('ciplv', phi, E)
    assert got[0] == 0 and got[1] == 0
    assert got[2] == 1e-3 / E and got[4] == 2e-3 / E          # |r| clipped to 1: the value is i
    assert abs(got[3] - 0.25 / np.sqrt(1 - 0.25)) <= 1e-15


def test_finalize_lag_rejects_bad_arguments():
    sums = np.zeros((3, 8, 4))
    phi = np.zeros((3, 8), dtype=np.complex128)
    for kind in ('pli2_unbiased', 'ppc'):
        for E in (0, 1):
            with pytest.raises(ValueError, match='at least 2 epochs'):
                finalize_lag(kind, phi if kind == 'ppc' else sums, E)
    for kind in ('coherence', 'plv', 'cross_sum', 'plv_sum', 'wPLI', None):
        with pytest.raises(ValueError, match='out must be one of'):
            finalize_lag(kind, sums, 5)
    with pytest.raises(ValueError, match=r'\(\.\.\., 4\)'):
        finalize_lag('wpli', np.zeros((3, 8, 2)), 5)


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    a = np.zeros((3, 4096))
    freqs = [1., 2., 3.]
    w = nw.Morse(1000)
    for decim in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match='decim'):
            w.lag_batch(a, a, freqs, decim=decim)
        with pytest.raises(ValueError, match='decim'):
            w.lag_connectivity_batch(x, freqs, decim=decim)
    for out in ('cwt', 'coherence', 'plv', 'cross_sum', 'plv_sum', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.lag_batch(a, a, freqs, out=out)
        with pytest.raises(ValueError, match='out must be one of'):
            w.lag_connectivity_batch(x, freqs, out=out)
    for b in (np.zeros((3, 4095)), np.zeros((2, 4096)), np.zeros(4096), np.zeros((3, 1, 4096))):
        with pytest.raises(ValueError, match='same'):
            w.lag_batch(a, b, freqs)
    with pytest.raises(ValueError, match='same'):
        w.lag_batch(np.float64(1.), np.float64(1.), freqs)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.lag_connectivity_batch(bad, freqs)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.lag_connectivity_batch(x, freqs, indices=idx)
    # the two measures that need E >= 2
    for out in ('pli2_unbiased', 'ppc'):
        with pytest.raises(ValueError, match='at least 2 epochs'):
            w.lag_batch(a[:1], a[:1], freqs, out=out)
        with pytest.raises(ValueError, match='at least 2 epochs'):
            w.lag_connectivity_batch(x[:1], freqs, out=out)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.wpli('a', 'b', freqs, decim=0)
    with pytest.raises(ValueError):
        ew.wpli('a', 'z', freqs)                                          # no such channel
    with pytest.raises(ValueError, match='decim'):
        ew.lag_connectivity(['a', 'b'], freqs, decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.lag_connectivity(['a', 'b'], freqs, method='coherence')
    with pytest.raises(ValueError, match='indices'):
        ew.lag_connectivity(['a', 'b'], freqs, indices=([0], [2]))        # positions in ch_names, not in the epochs
    with pytest.raises(ValueError):
        ew.lag_connectivity(['a', 'z'], freqs)
    assert w._cache is None and not w._plans
    # the older entry points still reject the new names
    with pytest.raises(ValueError, match='out must be one of'):
        w.cross_batch(a, a, freqs, out='wpli')
    with pytest.raises(ValueError, match='out must be one of'):
        w.connectivity_batch(x, freqs, out='wpli')
    assert w._cache is None and not w._plans


def test_the_pair_kernel_forms_no_lag_partials():
    for n in (512, 1000, 1024, 2048, 4096, 8192, 16384, 32768):
        for dtype in (L.NW_F32, L.NW_F64):
            for kind in (L.NW_MORSE, L.NW_MORLET, L.NW_SHANNON, L.NW_TABLE, L.NW_MEXICAN_HAT, L.NW_HAAR):
                assert L.pair_partials_supported(n, dtype, kind, L.NW_OUT_LAG_SUM) == 0, (n, dtype, kind)
