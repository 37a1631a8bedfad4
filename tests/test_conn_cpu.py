"""Multi-channel connectivity without a GPU: the host-only pair tiler (nw_conn_tiles: every pair in
one tile, tiles within the kernel's limits, all pairs of C channels in at most m (m + 1) / 2 tiles
with m = ceil(C / 8)), the numpy finaliser engine.finalize_conn, the argument checks of
WaveletBase.connectivity_batch / EpochsWavelet.connectivity (before any device work) and the new
constant of nw_stats.reduce_path."""
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
from ninwavelets_amd.engine import CONN_KINDS, CONN_OUTS, all_pairs, check_indices, finalize_conn, finalize_pair

OUTS = ['cross_sum', 'plv_sum', 'csd', 'coherency', 'coherence', 'imcoh', 'plv']


def check_tiling(nchan, ia, ib):
    """The invariants of one tiling; returns the tile count."""
    tile, ntiles, (kch, kpairs, ktile) = L.conn_tiles(nchan, ia, ib)
    assert (kch, kpairs, ktile) == (16, 64, 64)
    ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    assert tile.shape == ia.shape and tile.dtype == np.int32
    if ia.size == 0:
        assert ntiles == 0
        return 0
    # every pair in exactly one tile, and no tile empty
    assert tile.min() == 0 and tile.max() == ntiles - 1
    assert sorted(set(tile.tolist())) == list(range(ntiles))
    for t in range(ntiles):
        members = np.flatnonzero(tile == t)
        assert 1 <= members.size <= kpairs, (t, members.size)
        assert len(set(ia[members].tolist()) | set(ib[members].tolist())) <= kch, t
    return ntiles


@pytest.mark.parametrize('nchan', [2, 3, 8, 9, 17, 64])
def test_all_pairs_tile_within_the_bound(nchan):
    ia, ib = all_pairs(nchan)
    ra, rb = np.triu_indices(nchan, 1)
    assert ia.dtype == np.int32 and ib.dtype == np.int32
    assert np.array_equal(ia, ra) and np.array_equal(ib, rb)
    m = -(-nchan // 8)
    ntiles = check_tiling(nchan, ia, ib)
    assert 1 <= ntiles <= m * (m + 1) // 2, (nchan, ntiles)


def test_any_pair_list_tiles():
    rng = np.random.default_rng(5)
    nchan = 23
    ia, ib = all_pairs(nchan)
    # shuffled, with repeats, reversed pairs (a > b) and self pairs
    pick = rng.integers(0, ia.size, 400)
    a = np.concatenate([ia[pick], ib[pick[:150]], np.arange(nchan)])
    b = np.concatenate([ib[pick], ia[pick[:150]], np.arange(nchan)])
    perm = rng.permutation(a.size)
    a, b = a[perm], b[perm]
    assert np.any(a > b) and np.any(a == b)
    ntiles = check_tiling(nchan, a, b)
    assert ntiles >= -(-a.size // 64)
    # one seed channel against all of 40: 15 partners per tile (16 channels)
    seeds = np.zeros(40, dtype=np.int32)
    assert check_tiling(40, seeds, np.arange(40)) == 3
    # the same list tiles the same way whatever the order of its rows: the tile of a pair is a
    # function of the sorted list
    t1, n1, _ = L.conn_tiles(nchan, a, b)
    t2, n2, _ = L.conn_tiles(nchan, a[::-1], b[::-1])
    assert n1 == n2
    assert check_tiling(5, [], []) == 0


def test_tiler_rejects_bad_arguments():
    one = np.zeros(1, dtype=np.int32)
    for nchan, a, b in ((0, [0], [0]), (-3, [0], [0]), (4, [4], [0]), (4, [0], [4]), (4, [-1], [0]), (4, [0, 1], [1, -2])):
        with pytest.raises(ValueError):
            L.conn_tiles(nchan, a, b)
    with pytest.raises(ValueError, match='equal length'):
        L.conn_tiles(4, [0, 1], [1])
    nt = ctypes.c_int64()
    P = ctypes.c_void_p
    rc = L.lib().nw_conn_tiles(4, one.ctypes.data_as(P), one.ctypes.data_as(P), -1, None, ctypes.byref(nt), None)
    assert rc == L.NW_E_INVALID
    assert L.lib().nw_conn_tiles(4, one.ctypes.data_as(P), one.ctypes.data_as(P), 1, None, None, None) == L.NW_E_INVALID
    # tile_of_pair and limits may be NULL
    assert L.lib().nw_conn_tiles(4, one.ctypes.data_as(P), one.ctypes.data_as(P), 1, None, ctypes.byref(nt), None) == 0
    assert nt.value == 1


def test_tiler_and_block_order_under_asan(tmp_path):
    """tests/asan/conn_asan.cpp with nw_host.cpp under -fsanitize=address,undefined: the tiler's
    descriptors (slots, channel lists, output rows) on all-pairs, seed, random and degenerate lists,
    and the kernel's block order (conn_slot, nw_shape.h): one block per (unit, pair tile)."""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'conn_asan')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', '-pthread', os.path.join(ROOT, 'ninwavelets_amd', 'csrc', 'nw_host.cpp'),
                    os.path.join(ROOT, 'tests', 'asan', 'conn_asan.cpp'), '-o', exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def random_rows(seed, E=7, C=4, shape=(5, 33)):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((E, 1) + shape) + 1j * rng.standard_normal((E, 1) + shape)
    return 0.5 * common + rng.standard_normal((E, C) + shape) + 1j * rng.standard_normal((E, C) + shape)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_finalize_conn_matches_the_formulas(seed):
    E, C = 7, 4
    y = random_rows(seed, E, C)
    ia = np.array([0, 0, 1, 3, 2, 2], dtype=np.int32)
    ib = np.array([1, 2, 3, 1, 0, 2], dtype=np.int32)
    cross = np.sum(y[:, ia] * np.conj(y[:, ib]), axis=0)
    power = np.sum(np.abs(y) ** 2, axis=0)
    u = y / np.abs(y)
    phi = np.sum(u[:, ia] * np.conj(u[:, ib]), axis=0)
    den = np.sqrt(power[ia] * power[ib])
    want = {'csd': cross / E, 'coherency': cross / den, 'coherence': np.abs(cross / den),
            'imcoh': (cross / den).imag, 'plv': np.abs(phi) / E}
    for kind in OUTS:
        got = finalize_conn(kind, phi if CONN_OUTS[kind] == 'plv_sum' else cross, power, ia, ib, E)
        if kind == 'cross_sum':
            assert got[0] is cross and got[1] is power
            continue
        if kind == 'plv_sum':
            assert got is phi
            continue
        assert got.shape == (ia.size,) + y.shape[2:], kind
        assert got.dtype == (np.complex128 if kind in ('csd', 'coherency') else np.float64), kind
        # the self pair (2, 2) has imcoh exactly 0: compare it absolutely
        err = np.max(np.abs(got - want[kind])[:5] / np.abs(want[kind])[:5])
        assert err <= 1e-15, (kind, err)
        # pair by pair it is finalize_pair
        for p in range(ia.size):
            src = phi[p] if kind == 'plv' else np.stack([cross[p].real, cross[p].imag, power[ia[p]], power[ib[p]]], -1)
            assert np.array_equal(got[p], finalize_pair(kind, src, E)), (kind, p)
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_conn('wpli', cross, power, ia, ib, E)


def test_self_pair_has_coherence_one_and_imcoh_zero():
    rng = np.random.default_rng(3)
    power = np.sum(rng.standard_normal((6, 3, 4, 50)) ** 2, axis=0)       # (C, F, n)
    ia = ib = np.array([0, 2, 1], dtype=np.int32)
    cross = power[ia] + 0j                                                # S_aa = P_aa, real
    assert np.array_equal(finalize_conn('coherence', cross, power, ia, ib, 6), np.ones((3, 4, 50)))
    assert np.array_equal(finalize_conn('imcoh', cross, power, ia, ib, 6), np.zeros((3, 4, 50)))
    assert np.array_equal(finalize_conn('csd', cross, power, ia, ib, 6), power[ia] / 6 + 0j)


def test_check_indices():
    ia, ib = check_indices(None, 4)
    assert np.array_equal(ia, [0, 0, 0, 1, 1, 2]) and np.array_equal(ib, [1, 2, 3, 2, 3, 3])
    ia, ib = check_indices(([3, 0], [0, 3]), 4)
    assert ia.dtype == np.int32 and ib.dtype == np.int32 and ia.flags.c_contiguous
    ia, ib = check_indices(([], []), 4)
    assert ia.size == 0 and ib.size == 0
    for bad in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0.5], [1.]), ([[0]], [[1]]), 3, ([0],)):
        with pytest.raises(ValueError, match='indices'):
            check_indices(bad, 4)


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    freqs = [1., 2., 3.]
    w = nw.Morse(1000)
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.connectivity_batch(x, freqs, decim=decim)
    for out in ('cwt', 'power_mean', 'wpli', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.connectivity_batch(x, freqs, out=out)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.connectivity_batch(bad, freqs)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.connectivity_batch(x, freqs, indices=idx)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='decim'):
        ew.connectivity(['a', 'b'], freqs, decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.connectivity(['a', 'b'], freqs, method='wpli')
    with pytest.raises(ValueError, match='indices'):
        ew.connectivity(['a', 'b'], freqs, indices=([0], [2]))        # positions in ch_names, not in the epochs
    with pytest.raises(ValueError):
        ew.connectivity(['a', 'z'], freqs)                            # no such channel
    assert w._cache is None and not w._plans


def test_constants():
    assert L.NW_REDUCE_CONN == 3
    assert (L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS) == (0, 1, 2)
    assert L.nw_stats._fields_[-1][0] == 'reduce_path'
    assert CONN_KINDS == {'cross_sum': L.NW_OUT_CROSS_SUM, 'plv_sum': L.NW_OUT_PLV_SUM}
    assert sorted(CONN_OUTS) == sorted(OUTS)
