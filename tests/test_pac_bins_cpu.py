"""Phase-binned phase-amplitude coupling without a GPU: the numpy finaliser engine.finalize_pac_bins against
formulas written out directly (and its empty-bin, zero-sum and P_b = 0 conventions), the edge table nw_pac_bin_edges
and the bin rule on it against atan2 binning and at its documented special points, the kernel's block map, tile
geometry and LDS bytes (nw_shape.h, a stand-alone host program), the argument checks that fire before any device
work, and the new constants, exports and signatures."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from epoch_cases import FakeEpochs
from pac_bins_cases import atan2_bin, bin_of, binned_sums

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import PAC_BIN_OUTS, PAC_OUTS, check_nbins, finalize_pac_bins

KINDS = ('bin_amp', 'mi', 'hr', 'pref_phase')


def test_block_map_tile_geometry_and_lds_on_the_host(tmp_path):
    """tests/asan/pac_bins_shape.cpp (a stand-alone program over nw_shape.h) under -fsanitize=address,undefined:
    one block per (epoch, pair, listed phase scale, amplitude tile) in both block orders, every listed scale
    combination in exactly one tile, partial tiles included, for every nbins class; the LDS of a block for
    nbins = 2, 18, 36 (and every other valid nbins) is <= 163840 bytes."""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'pac_bins_shape')
    subprocess.run([gxx, '-std=c++20', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'asan', 'pac_bins_shape.cpp'), '-o', exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='hipcc not available')
def test_diagnostic_switches_compile(tmp_path):
    """The three A/B builds tools/pac_bins_rate.py was measured on still build, each switch on its own as it was
    measured (device-only compiles side by side, nothing runs), as tests/test_diag_builds.py does for the other kernels."""
    src = os.path.join(ROOT, 'ninwavelets_amd', 'csrc', 'nw_pac_bins.hip')
    procs = [(d, subprocess.Popen(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++20', '--cuda-device-only',
                                   f'-D{d}', '-c', src, '-o', str(tmp_path / (d + '.co'))],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
             for d in ('NW_ABL_PACBINS_NOHYPOT', 'NW_ABL_PACBINS_NOBIN', 'NW_ABL_PACBINS_NOLDS')]
    for d, p in procs:
        _, err = p.communicate(timeout=120)
        assert p.returncode == 0, f'{d}: {err[-2000:]}'
        assert os.path.getsize(tmp_path / (d + '.co')) > 0


def _direct(S, count, ip):
    """bin_amp, mi, hr and pref_phase cell by cell, as the formulas read (no empty bin, a positive total)."""
    E, P, Fp, Fa, nb = S.shape
    amp = np.empty(S.shape)
    mi, hr, pref = (np.empty(S.shape[:-1]) for _ in range(3))
    for e in range(E):
        for p in range(P):
            for i in range(Fp):
                for k in range(Fa):
                    A = S[e, p, i, k] / count[e, ip[p], i]
                    Pb = A / A.sum()
                    amp[e, p, i, k] = A
                    mi[e, p, i, k] = (np.log(nb) + sum(q * np.log(q) for q in Pb if q > 0)) / np.log(nb)
                    hr[e, p, i, k] = (Pb.max() - Pb.min()) / Pb.max()
                    pref[e, p, i, k] = -np.pi + 2 * np.pi * int(np.argmax(A)) / nb + np.pi / nb
    return {'bin_amp': amp, 'mi': mi, 'hr': hr, 'pref_phase': pref}


def test_finalize_pac_bins_against_direct_formulas():
    rng = np.random.default_rng(19)
    E, C, F, T, nb = 2, 3, 6, 400, 18
    y = rng.standard_normal((E, C, F, T)) + 1j * rng.standard_normal((E, C, F, T))
    fph, fam = [0, 1, 1], [2, 5, 3, 2]
    ip, ia = np.array([0, 2, 1, 1]), np.array([1, 0, 1, 2])
    S, count, bins, A = binned_sums(y, ip, ia, fph, fam, np.arange(T), nb, False)
    assert count.min() >= 1 and np.array_equal(count.sum(-1), np.full((E, C, len(fph)), float(T)))
    want = _direct(S, count, ip)
    assert set(want) | {'bin_sum'} == set(PAC_BIN_OUTS)
    for kind, ref in want.items():
        got = finalize_pac_bins(kind, S, count, ip)
        assert got.shape == ref.shape and got.dtype == np.float64, kind
        assert np.allclose(got, ref, rtol=1e-12, atol=1e-15), kind
    mi, hr = finalize_pac_bins('mi', S, count, ip), finalize_pac_bins('hr', S, count, ip)
    assert mi.min() >= 0 and mi.max() <= 1 and hr.min() >= 0 and hr.max() <= 1
    # the sums pass through unchanged
    got = finalize_pac_bins('bin_sum', S, count, ip)
    assert got[0] is S and got[1] is count
    with pytest.raises(ValueError, match='out must be one of'):
        finalize_pac_bins('direct_pac', S, count, ip)
    with pytest.raises(ValueError, match='shapes'):
        finalize_pac_bins('mi', S[..., 0], count, ip)
    with pytest.raises(ValueError, match='shapes'):
        finalize_pac_bins('mi', S, count[..., :4], ip)
    # empty epoch and pair axes keep their shapes
    for kind in KINDS:
        tail = (nb,) if kind == 'bin_amp' else ()
        assert finalize_pac_bins(kind, S[:0], count[:0], ip).shape == (0, len(ip), len(fph), len(fam)) + tail
        assert finalize_pac_bins(kind, S[:, :0], count, ip[:0]).shape == (E, 0, len(fph), len(fam)) + tail


def test_finalize_pac_bins_conventions():
    nb = 6
    S = np.zeros((1, 2, 1, 3, nb))
    count = np.full((1, 2, 1, nb), 5.)
    ip = [0, 1]
    # a uniform distribution: mi = hr = 0; a single occupied bin: mi = hr = 1, its P_b = 0 terms adding 0
    S[0, :, 0, 0] = 10.
    S[0, :, 0, 1, 4] = 7.
    # cell 2 stays all zero: sum_b A_b = 0 with no empty bin -> mi = hr = 0, not NaN
    mi, hr = finalize_pac_bins('mi', S, count, ip), finalize_pac_bins('hr', S, count, ip)
    assert np.allclose(mi[0, :, 0, 0], 0., atol=1e-15) and np.array_equal(hr[0, :, 0, 0], [0., 0.])
    assert np.allclose(mi[0, :, 0, 1], 1., atol=1e-15) and np.array_equal(hr[0, :, 0, 1], [1., 1.])
    assert np.array_equal(mi[0, :, 0, 2], [0., 0.]) and np.array_equal(hr[0, :, 0, 2], [0., 0.])
    pref = finalize_pac_bins('pref_phase', S, count, ip)
    assert np.allclose(pref[0, :, 0, 1], -np.pi + 2 * np.pi * 4 / nb + np.pi / nb)
    assert np.allclose(pref[0, :, 0, 0], -np.pi + np.pi / nb)     # a tie: the first bin
    assert np.array_equal(finalize_pac_bins('bin_amp', S, count, ip)[0, 0, 0, 1], [0, 0, 0, 0, 7. / 5., 0])
    # an empty bin of the phase channel of pair 1 only: NaN there in bin_amp, the whole cell NaN in the measures
    count[0, 1, 0, 2] = 0.
    amp = finalize_pac_bins('bin_amp', S, count, ip)
    assert np.isnan(amp[0, 1, 0, :, 2]).all() and not np.isnan(amp[0, 0]).any() and not np.isnan(amp[0, 1, 0, :, :2]).any()
    for kind in ('mi', 'hr', 'pref_phase'):
        got = finalize_pac_bins(kind, S, count, ip)
        assert np.isnan(got[0, 1]).all() and not np.isnan(got[0, 0]).any(), kind
    # the counts are the PHASE channel's: pair (1, 0) reads channel 1's counts
    assert np.isnan(finalize_pac_bins('mi', S, count, [1, 0])[0, 0]).all()
    # pref_phase on a planted histogram: a cosine bump centred on bin 13 of 18
    nb = 18
    centres = -np.pi + 2 * np.pi * np.arange(nb) / nb + np.pi / nb
    S = (2. + np.cos(centres - centres[13]))[None, None, None, None, :] * 7.
    count = np.full((1, 1, 1, nb), 7.)
    assert finalize_pac_bins('pref_phase', S, count, [0])[0, 0, 0, 0] == centres[13]
    assert 0 < finalize_pac_bins('mi', S, count, [0])[0, 0, 0, 0] < finalize_pac_bins('hr', S, count, [0])[0, 0, 0, 0] < 1


def test_edge_table_and_its_errors():
    for nb in (2, 4, 18, 36):
        cs = L.pac_bin_edges(nb)
        assert cs.shape == (nb, 2) and cs.dtype == np.float64
        theta = -np.pi + 2 * np.pi * np.arange(nb) / nb
        assert np.allclose(cs[:, 0], np.cos(theta), rtol=0, atol=1e-15) and np.allclose(cs[:, 1], np.sin(theta), rtol=0, atol=1e-15)
        assert cs[0, 0] == -1. and cs[nb // 2, 0] == 1. and abs(cs[nb // 2, 1]) <= 1e-15
    buf = np.empty((40, 2))
    for bad in (0, 1, 3, 17, 37, 38, -2):
        assert L.lib().nw_pac_bin_edges(bad, buf.ctypes.data_as(ctypes.c_void_p)) == L.NW_E_INVALID
        assert f'nbins ({bad})'.encode() in L.lib().nw_last_error(), L.lib().nw_last_error()
    assert L.lib().nw_pac_bin_edges(18, None) == L.NW_E_INVALID
    for bad in (0, 1, 3, 38, -2, 2.5, None, 'x', True):
        with pytest.raises(ValueError, match='nbins'):
            L.pac_bin_edges(bad)
        with pytest.raises(ValueError, match='nbins'):
            check_nbins(bad)
    assert check_nbins(np.int64(18)) == 18 and check_nbins(2) == 2 and check_nbins(36) == 36


def test_bin_rule_against_atan2_and_at_its_special_points():
    rng = np.random.default_rng(23)
    for nb in (2, 4, 6, 18, 36):
        h = nb // 2
        # random points whose angle lies at least 1e-9 from every edge
        phi = rng.uniform(-np.pi, np.pi, 20000)
        width = 2 * np.pi / nb
        off = (phi + np.pi) % width
        phi = phi[(off > 1e-9) & (off < width - 1e-9)]
        r = np.exp(rng.uniform(-30., 30., phi.size))
        re, im = r * np.cos(phi), r * np.sin(phi)
        assert np.array_equal(bin_of(re, im, nb), atan2_bin(re, im, nb)), nb
        assert np.array_equal(bin_of(re, im, nb), np.floor((phi + np.pi) / width)), nb
        # the documented special points
        z, nan, inf = 0., float('nan'), float('inf')
        assert bin_of(-1., z, nb) == 0 and bin_of(-1., -z, nb) == 0            # re < 0, im = +-0: bin 0
        assert bin_of(z, z, nb) == h and bin_of(-z, z, nb) == h and bin_of(z, -z, nb) == h and bin_of(-z, -z, nb) == h
        assert bin_of(1., z, nb) == h and bin_of(1., -z, nb) == h              # the positive real axis: theta_h = 0
        for a, b in ((nan, nan), (1., nan), (-1., nan), (nan, z), (nan, -1.)):
            assert bin_of(a, b, nb) == 0                                       # NaN: every comparison is false
        assert bin_of(nan, 1., nb) == h                                        # ... but im > 0: the upper half's first
        assert 0 <= bin_of(inf, 1., nb) < nb and 0 <= bin_of(-inf, -inf, nb) < nb
        if nb % 4:                                                             # the imaginary axis is no edge
            assert bin_of(z, 1., nb) == atan2_bin(z, 1., nb) and bin_of(z, -1., nb) == atan2_bin(z, -1., nb)
        # every bin is hit, in order, by its centre
        centres = -np.pi + width * (np.arange(nb) + 0.5)
        assert np.array_equal(bin_of(np.cos(centres), np.sin(centres), nb), np.arange(nb))


def test_bad_arguments_are_value_errors_before_any_device_work():
    """No device is touched: the checks come before the cache build and the plan."""
    x = np.zeros((3, 4, 4096))
    freqs = [4., 7., 12., 40., 70.]
    w = nw.Morse(1000)
    ok = dict(phase=[0, 1], amp=[3, 4])
    for nbins in (0, 1, 3, 17, 38, -2, 2.5, None, '18', True):
        with pytest.raises(ValueError, match='nbins'):
            w.pac_bins_batch(x, freqs, nbins=nbins, **ok)
    for decim in (0, -2, 2.5):
        with pytest.raises(ValueError, match='decim'):
            w.pac_bins_batch(x, freqs, decim=decim, **ok)
    for out in ('cwt', 'direct_pac', 'pac_sum', None):
        with pytest.raises(ValueError, match='out must be one of'):
            w.pac_bins_batch(x, freqs, out=out, **ok)
    for out in ('bin_sum', 'pref_phase'):
        with pytest.raises(ValueError, match='average'):
            w.pac_bins_batch(x, freqs, out=out, average=True, **ok)
    for bad in (np.zeros(4096), np.zeros((3, 4096)), np.zeros((2, 3, 4, 4096)), np.float64(1.)):
        with pytest.raises(ValueError, match='epochs, channels'):
            w.pac_bins_batch(bad, freqs, **ok)
    for idx in (([0, 1], [1]), ([0], [4]), ([-1], [0]), ([0, 1, 2], [1, 2, 9])):
        with pytest.raises(ValueError, match='indices'):
            w.pac_bins_batch(x, freqs, indices=idx, **ok)
    for bad in ([5], [-1], [0, 7], [], None, [1.5]):              # scale positions out of range, empty lists
        with pytest.raises(ValueError, match='phase'):
            w.pac_bins_batch(x, freqs, phase=bad, amp=[3, 4])
        with pytest.raises(ValueError, match='amp'):
            w.pac_bins_batch(x, freqs, phase=[0, 1], amp=bad)
    with pytest.raises(ValueError, match='phase'):                # the defaults are no lists
        w.pac_bins_batch(x, freqs)
    for win in ((-1, 5), (6, 5), (0, 4097), (0.5, 3), (1,), 7):
        with pytest.raises(ValueError, match='window'):
            w.pac_bins_batch(x, freqs, window=win, **ok)
    for kind in KINDS:                                            # an empty window has no finalised measure
        with pytest.raises(ValueError, match='at least 1'):
            w.pac_bins_batch(x, freqs, out=kind, window=(8, 8), **ok)
        with pytest.raises(ValueError, match='at least 1'):
            w.pac_bins_batch(x, freqs, out=kind, window=(1, 4), decim=4, **ok)
    ew = nw.EpochsWavelet(FakeEpochs(np.zeros((3, 3, 4096)), 1000., ['a', 'b', 'c']), w)
    with pytest.raises(ValueError, match='nbins'):
        ew.pac_bins(['a', 'b'], [4., 7.], [40., 70.], nbins=5)
    with pytest.raises(ValueError, match='decim'):
        ew.pac_bins(['a', 'b'], [4., 7.], [40., 70.], decim=0)
    with pytest.raises(ValueError, match='out must be one of'):
        ew.pac_bins(['a', 'b'], [4., 7.], [40., 70.], method='mvl')
    with pytest.raises(ValueError, match='indices'):
        ew.pac_bins(['a', 'b'], [4., 7.], [40., 70.], indices=([0], [2]))
    with pytest.raises(ValueError):
        ew.pac_bins(['a', 'z'], [4., 7.], [40., 70.])             # no such channel
    with pytest.raises(ValueError, match='phase'):
        ew.pac_bins(['a', 'b'], [], [40., 70.])
    with pytest.raises(ValueError, match='amp'):
        ew.pac_bins(['a', 'b'], [4., 7.], [])
    for padding in (2.048, 3., -0.1, float('nan')):
        with pytest.raises(ValueError, match='padding'):
            ew.pac_bins(['a', 'b'], [4., 7.], [40., 70.], padding=padding)
    with pytest.raises(ValueError, match='average'):
        ew.pac_bins(['a', 'b'], [4., 7.], [40., 70.], method='pref_phase', average=True)
    assert w._cache is None and not w._plans


def test_constants_and_exports():
    assert L.NW_REDUCE_PAC_BINS == 7 and L.NW_PAC_MAX_BINS == 36
    assert {L.NW_REDUCE_NONE, L.NW_REDUCE_ROWS, L.NW_REDUCE_PARTIALS, L.NW_REDUCE_CONN, L.NW_REDUCE_CONN_TIME,
            L.NW_REDUCE_PAC, L.NW_REDUCE_ENV, L.NW_REDUCE_PAC_BINS} == set(range(8))
    assert PAC_BIN_OUTS == {'bin_sum', 'bin_amp', 'mi', 'hr', 'pref_phase'}
    assert PAC_OUTS == {'pac_sum', 'mvl', 'mvl_norm', 'direct_pac', 'debiased_pac'}          # left alone
    assert nw.finalize_pac_bins is finalize_pac_bins and 'finalize_pac_bins' in nw.__all__
    assert hasattr(nw.Plan, 'execute_pac_bins') and hasattr(nw.WaveletBase, 'pac_bins_batch')
    assert hasattr(nw.EpochsWavelet, 'pac_bins')
    sig = {s[0]: s for s in L.SIGNATURES}
    assert len(sig['nw_execute_pac'][2]) == 18                    # untouched
    assert len(sig['nw_execute_pac_bins'][2]) == 18 and len(sig['nw_pac_bin_edges'][2]) == 2
    with open(os.path.join(ROOT, 'include', 'ninwave.h')) as f:
        header = f.read()
    assert '#define NW_PAC_MAX_BINS 36' in header and '#define NW_REDUCE_PAC_BINS 7' in header
    assert 'int nw_pac_bin_edges(int32_t nbins, double* cs);' in header and 'int nw_execute_pac_bins(' in header
    assert 'THE BIN' in header and 'no atan2' in header
    assert hasattr(L.lib(), 'nw_execute_pac_bins') and hasattr(L.lib(), 'nw_pac_bin_edges')   # host-only load
