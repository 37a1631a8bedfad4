"""Cross-channel pair reductions without a GPU: the numpy finalisers (engine.finalize_pair), the
argument checks of the class API (before any device work) and the host-only predicate
nw_pair_partials_supported, whose set is read from the decision lines of
profiles/r11_pair_rate.txt."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FakeEpochs

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import PAIR_KINDS, PAIR_OUTS, finalize_pair

OUTS = ['cross_sum', 'plv_sum', 'csd', 'coherency', 'coherence', 'imcoh', 'plv']
SIZES = (1024, 2048, 4096)          # the sizes the fused pair partials may cover, at most


def random_sums(seed, shape=(5, 33)):
    """Sums as E random pairs of complex rows give them (so |S_ab|^2 <= P_aa P_bb holds)."""
    rng = np.random.default_rng(seed)
    E = 7
    ya = rng.standard_normal((E,) + shape) + 1j * rng.standard_normal((E,) + shape)
    yb = 0.5 * ya + rng.standard_normal((E,) + shape) + 1j * rng.standard_normal((E,) + shape)
    s = np.sum(ya * np.conj(yb), axis=0)
    cross = np.stack([s.real, s.imag, np.sum(np.abs(ya) ** 2, axis=0), np.sum(np.abs(yb) ** 2, axis=0)], axis=-1)
    phi = np.sum(ya / np.abs(ya) * np.conj(yb / np.abs(yb)), axis=0)
    return E, cross, phi


def test_pair_outs_are_the_issue_s():
    assert sorted(PAIR_OUTS) == sorted(OUTS)
    assert PAIR_KINDS == {'cross_sum': 7, 'plv_sum': 8}
    assert (L.NW_OUT_CROSS_SUM, L.NW_OUT_PLV_SUM) == (7, 8)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_finalize_pair_matches_the_formulas(seed):
    E, cross, phi = random_sums(seed)
    s = cross[..., 0] + 1j * cross[..., 1]
    paa, pbb = cross[..., 2], cross[..., 3]
    want = {'cross_sum': cross, 'plv_sum': phi, 'csd': s / E, 'coherency': s / np.sqrt(paa * pbb),
            'coherence': np.abs(s / np.sqrt(paa * pbb)), 'imcoh': (s / np.sqrt(paa * pbb)).imag,
            'plv': np.abs(phi) / E}
    for kind in OUTS:
        got = finalize_pair(kind, phi if PAIR_OUTS[kind] == 'plv_sum' else cross, E)
        assert got.shape == want[kind].shape, kind
        assert got.dtype == (np.complex128 if kind in ('plv_sum', 'csd', 'coherency') else np.float64), kind
        err = np.max(np.abs(got - want[kind]) / np.abs(want[kind]))
        assert err <= 1e-15, (kind, err)
    assert np.all(finalize_pair('coherence', cross, E) <= 1 + 1e-15)
    assert np.all(finalize_pair('plv', phi, E) <= 1 + 1e-15)
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_pair('wpli', cross, E)


def test_coherence_of_a_channel_with_itself_is_one():
    rng = np.random.default_rng(3)
    p = np.sum(rng.standard_normal((6, 4, 50)) ** 2, axis=0)         # exact sums: S_aa = P_aa, real
    cross = np.stack([p, np.zeros_like(p), p, p], axis=-1)
    assert np.array_equal(finalize_pair('coherence', cross, 6), np.ones_like(p))
    assert np.array_equal(finalize_pair('imcoh', cross, 6), np.zeros_like(p))
    assert np.array_equal(finalize_pair('csd', cross, 6), p / 6 + 0j)


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    a = np.zeros((3, 4096))
    freqs = [1., 2., 3.]
    w = nw.Morse(1000)
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.cross_batch(a, a, freqs, decim=decim)
    for out in ('cwt', 'power_mean', 'wpli', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.cross_batch(a, a, freqs, out=out)
    for b in (np.zeros((2, 4096)), np.zeros((3, 2048)), np.zeros(4096), np.zeros((3, 1, 4096))):
        with pytest.raises(ValueError, match='same'):
            w.cross_batch(a, b, freqs)
    with pytest.raises(ValueError, match='same'):
        w.cross_batch(np.float64(1.), np.float64(2.), freqs)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 2, 4096)), 1000., ['a', 'b']), w)
    for call in (ew.csd, ew.coherence, ew.imcoh, ew.plv):
        with pytest.raises(ValueError, match='decim'):
            call('a', 'b', freqs, decim=0)
    assert w._cache is None and not w._plans


def decided_sizes():
    """{'cross_sum': sizes, 'plv_sum': sizes} of the lines 'decision <kind>: <n> <n> ...' (or
    'none') of profiles/r11_pair_rate.txt."""
    text = open(os.path.join(ROOT, 'profiles', 'r11_pair_rate.txt')).read()
    found = dict(re.findall(r'^decision (cross_sum|plv_sum):\s*(.*?)\s*$', text, flags=re.M))
    assert sorted(found) == ['cross_sum', 'plv_sum'], found
    return {k: set() if v == 'none' else {int(t) for t in v.split()} for k, v in found.items()}


def test_pair_partials_supported_table():
    keep = decided_sizes()
    for kind, sizes in keep.items():
        assert sizes <= set(SIZES), (kind, sizes)
    analytic = (L.NW_MORSE, L.NW_MORLET, L.NW_SHANNON)
    out_of = {'cross_sum': L.NW_OUT_CROSS_SUM, 'plv_sum': L.NW_OUT_PLV_SUM}
    lengths = [512 << i for i in range(7)] + [1000, 1201, 3000, 4095, 4097]
    for n in lengths:
        for kind in analytic + (L.NW_TABLE, L.NW_MEXICAN_HAT, L.NW_HAAR):
            for name, ok in out_of.items():
                assert not L.pair_partials_supported(n, L.NW_F64, kind, ok), (n, kind, name)
                want = n in keep[name] and kind in analytic
                assert L.pair_partials_supported(n, L.NW_F32, kind, ok) == want, (n, kind, name)
            for other in (L.NW_OUT_CWT, L.NW_OUT_POWER, L.NW_OUT_POWER_SUM, L.NW_OUT_PHASE_SUM, 9, -1):
                assert not L.pair_partials_supported(n, L.NW_F32, kind, other), (n, kind, other)
    assert not L.pair_partials_supported(4096, 7, L.NW_MORSE, L.NW_OUT_CROSS_SUM)      # not a compute dtype


def test_stats_structure_ends_with_reduce_path():
    assert L.nw_stats._fields_[-1][0] == 'reduce_path'
    assert (L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS) == (0, 1, 2)
