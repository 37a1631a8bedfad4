"""CPU checks of tests/aux_cases.py, the cases of the wavelet-row, time-domain-wavelet, Normal-table and baseline
GPU tests: the fp32 floor the row bound rests on (measured from the numpy restatement of psi_f32, written to the
record), that the sweeps reach the paths they are there for (asserted on the oracle alone), and the row lengths
nw_make_wavelets reports before it opens a device."""
import ctypes

import numpy as np
import pytest

import aux_cases as A
from oracle import nw_oracle as O

from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import KINDS

FLOOR_MAX = 5e-6


@pytest.mark.parametrize('case', A.ROW_SETS, ids=A.set_id)
def test_fp32_floor(case):
    """The float32 restatement of psi_f32 stays within 5e-6 of each row's peak on the 40 scales at n = 4096."""
    rows = A.floor_rows(*case)
    assert np.all(np.isfinite(rows))           # every oracle row of a listed set is finite
    floor = A.floor_of(*case)
    print(f'{A.set_id(case)}: floor {floor:.3e}')
    assert floor == rows.max() and floor <= FLOOR_MAX


def test_fp32_floor_of_the_overflow_set():
    """Morse b = 100, r = 3: the floor over the scales whose oracle row is finite, and both kinds of row among the
    four scales test_gpu_wavelet_rows.py runs it on."""
    rows = A.floor_rows(*A.OVERFLOW_SET)
    assert 0 < np.isnan(rows).sum() < len(rows)
    assert A.floor_of(*A.OVERFLOW_SET) <= FLOOR_MAX
    with np.errstate(all='ignore'):
        ref = O.fft_wavelets('morse', A.OVERFLOW_FREQS, 1000., A.ROW_N / 1000., False, b=100., r=3.)
    finite = [bool(np.all(np.isfinite(r))) for r in ref]
    assert finite == [False, False, True, True]


def test_fp32_floor_table_is_recorded():
    """The floors and the scale each is reached at, as test_gpu_wavelet_rows.py uses them (bound = 4 floor + 2^-23)."""
    lines = ['# max over FREQS40 of max_j |psi32_restated - oracle| / row peak, n = 4096, sfreq 1000 (numpy float32)',
             f'{"set":<22}{"floor":>12}{"at f (Hz)":>12}{"fp32 row bound":>16}']
    for case in A.ROW_SETS + [A.OVERFLOW_SET]:        # (the last: over its finite rows)
        rows = A.floor_rows(*case)
        i = int(np.nanargmax(rows))
        assert rows[i] == A.floor_of(*case)
        lines.append(f'{A.set_id(case):<22}{rows[i]:>12.3e}{A.FREQS40[i]:>12.3f}{4 * rows[i] + 2.0 ** -23:>16.3e}')
    A.record('1. fp32 floors (test_aux_cases_cpu.py::test_fp32_floor_table_is_recorded)', lines)


def test_restatement_is_float32_and_zero_at_dc():
    for case in A.ROW_SETS:
        v = A.psi32_restated(*case, np.arange(8), 1000 / 4096, 7.)
        assert v.dtype == np.float32 and np.all(np.isfinite(v))
        if case[0] == 'morse':
            assert v[0] == 0


def lens_of(name, sfreq, rwl):
    return {len(r) for r in A.sweep_oracle(name, A.SWEEP_FREQS, sfreq, rwl)}


def test_sweep_reaches_the_untested_paths():
    """On the oracle alone: odd m in the conj-flip slice, rows of two lengths in one call (one rocFFT plan per
    length, the non-smooth 999 among them), and two row lengths in every Normal-table case."""
    for name in ('morse', 'morse_b3_r2', 'shannon'):
        assert lens_of(name, 999, 1) == {998, 1000}
        assert lens_of(name, 1001, 1) == {1000, 1002}
        assert {A.reverse_m(f, 999, 1) for f in A.SWEEP_FREQS} == {999, 1000}          # odd m; rocFFT length 999
        assert {A.reverse_m(f, 1001, 1) for f in A.SWEEP_FREQS} == {1001, 1002}
        assert {A.reverse_m(f, 1000, 0.301) for f in A.SWEEP_FREQS} == {301}           # odd m alone
    for name in ('morlet_s5', 'mexican_hat'):
        assert lens_of(name, 1000, 1) == {1000, 1001}
    for case in A.NORMAL_CASES:
        for name in A.NORMAL_KINDS:
            for interpolate in (False, True):
                lens = {len(r) for r in A.normal_oracle_rows(name, *case, interpolate)}
                assert len(lens) == 2, (case, name, lens)


def device_free_lengths(kind, params, freqs, sfreq, rwl):
    """The row lengths of nw_make_wavelets' sizing call (out = NULL), which returns before a device is opened."""
    fr = np.ascontiguousarray(freqs, dtype=np.float64)
    p = np.ascontiguousarray(params, dtype=np.float64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    lens = np.full(fr.size, -1, dtype=np.int64)
    mx = ctypes.c_int64(-1)
    L.check(L.lib().nw_make_wavelets(0, KINDS[kind], p.ctypes.data_as(dp), int(p.size), fr.ctypes.data_as(dp),
                                     int(fr.size), float(sfreq), float(rwl), None, ctypes.byref(mx),
                                     lens.ctypes.data_as(ip)))
    assert mx.value == lens.max()
    return lens


@pytest.mark.parametrize('name', list(A.SWEEP_KINDS))
def test_lengths_without_a_device(name):
    """Over 30 sampling rates in [97, 2003], three real_wave_length and FREQS40, the lengths equal the oracle's."""
    bad = []
    for sfreq in np.linspace(97., 2003., 30):
        for rwl in (0.301, 1, 1.5):
            w = A.sweep_wavelet(name, float(sfreq), rwl)
            kind, params = w._device_wavelet_spec()
            got = device_free_lengths(kind, params, A.FREQS40, sfreq, rwl)
            want = [len(r) for r in A.sweep_oracle(name, A.FREQS40, float(sfreq), rwl)]
            bad += [(float(sfreq), rwl, float(f), int(g), e) for f, g, e in zip(A.FREQS40, got, want) if g != e]
    assert not bad, bad[:10]
