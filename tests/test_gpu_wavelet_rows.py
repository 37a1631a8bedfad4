"""GPU parity of the wavelet row evaluators psi_f64 / psi_f32 (nw_internal.h) through k_rows (nw_kernels.hip), which
also fill the W tables of the one-pass and chirp kernels: Plan.rows() of a plan at n = 4096 against
oracle.nw_oracle.fft_wavelets, for every parameter set of tests/aux_cases.py, in both dtypes, on three grids:

  full    trans_grid(n / 1000, 1000, False)
  interp  the same with interpolate True (len_full = 2 len_valid, the upper half exactly 0)
  half    trans_grid(n / 2000, 1000, False): a cache built for another length, twice the spacing

Bounds.  fp64: max |d| <= 1e-13 max(1, row peak) per row (test_gpu_parity.py's
test_device_wavelet_rows_match_reference).  fp32: per parameter set, max |d| / row peak <= 4 floor + 2^-23 with floor
= aux_cases.floor_of, the error of the numpy float32 restatement of psi_f32 on the 40 scales (CPU arithmetic only;
test_aux_cases_cpu.py holds it to 5e-6).  The factor 4 is a chosen margin: the device's v_log_f32 / v_exp_f32 are
1-ulp instructions against numpy's half-ulp log2 / exp2, on both transcendentals of the exponent; 2^-23 is one
rounding of the result at the peak.

Then Shannon (exact rows, nu = 1.0 on a bin: the <= edge), Morse b = 100 (the rows that hold inf / NaN bins are the
oracle's) and one CWT per non-default family through the one-pass, chirp and decimated forms, every (signal, scale)
row against its own maximum."""
import numpy as np
import pytest

import aux_cases as A
from epoch_cases import FREQS, tol_of
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

N = A.ROW_N
GRIDS = {'full': (N / 1000., False), 'interp': (N / 1000., True), 'half': (N / 2000., False)}
DTYPES = ['float64', 'float32']
MEASURED = {}                       # (set id, dtype, grid) -> the largest |d| / bound unit, for the record


def device_rows(kind, params, freqs, dtype, real_length, interpolate, n=N):
    p = nw.Plan(n, len(freqs), dtype, interpolate=interpolate)
    try:
        p.set_wavelet(kind, A.plan_params(kind, params), np.asarray(freqs, dtype=np.float64),
                      L.trans_grid(real_length, 1000., interpolate))
        return p.rows()
    finally:
        p.close()


def oracle_rows(kind, params, freqs, real_length, interpolate):
    with np.errstate(all='ignore'):
        return np.array(O.fft_wavelets(kind, freqs, 1000., real_length, interpolate, **A.oracle_params(kind, params)))


def fp32_bound(kind, params):
    return 4 * A.floor_of(kind, params) + 2.0 ** -23


def row_errors(got, ref, dtype):
    """Per row, max |d| in the bound's unit: max(1, row peak) in fp64, the row peak in fp32."""
    peak = np.max(np.abs(ref), axis=1)
    unit = np.maximum(1.0, peak) if dtype == 'float64' else peak
    return np.max(np.abs(got.astype(np.float64) - ref), axis=1) / unit


@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', A.ROW_SETS, ids=A.set_id)
def test_rows_against_the_oracle(case, dtype, grid):
    kind, params = case
    rl, interp = GRIDS[grid]
    ref = oracle_rows(kind, params, A.FREQS40, rl, interp)
    got = device_rows(kind, params, A.FREQS40, dtype, rl, interp)
    assert got.shape == ref.shape and got.dtype == np.dtype(dtype)
    assert ref.shape[1] == (N if grid != 'half' else N // 2)
    if interp:
        assert np.all(got[:, ref.shape[1] // 2:] == 0)              # exactly zero, not merely small
    err = row_errors(got, ref, dtype)
    bound = 1e-13 if dtype == 'float64' else fp32_bound(kind, params)
    worst = float(err.max())
    MEASURED[(A.set_id(case), dtype, grid)] = worst
    print(f'{A.set_id(case)} {dtype} {grid}: worst {worst:.3e} at {A.FREQS40[int(err.argmax())]:.3f} Hz, bound {bound:.3e}'
          + (f' = 4 x {A.floor_of(kind, params):.3e} + 2^-23, ratio to floor {worst / A.floor_of(kind, params):.2f}'
             if dtype == 'float32' else ''))
    assert worst <= bound, (A.set_id(case), dtype, grid, worst, bound)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [4000, 4096])
def test_shannon_rows_are_exact(n, dtype):
    """n = 4000: delta = 0.25, so nu = 1.0 falls exactly on bin 4 (the `<=` edge); on the half grid on bin 2."""
    for rl, interp in ((n / 1000., False), (n / 1000., True), (n / 2000., False)):
        ref = oracle_rows('shannon', (), FREQS, rl, interp)
        got = device_rows('shannon', (), FREQS, dtype, rl, interp, n=n)
        assert got.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(got, ref)
        if n == 4000:
            edge = 4 if rl == n / 1000. else 2
            assert np.all(ref[:, edge] == 1) and np.all(ref[:, edge + 1] == 0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_morse_overflow_rows(dtype):
    """Morse b = 100, r = 3: x^b overflows the reference's fp64 at the two low scales (inf, and NaN where the exp
    term has underflowed to 0).  The rows holding a non-finite bin are the oracle's; finite rows meet the bounds."""
    kind, params = A.OVERFLOW_SET
    rl, interp = GRIDS['full']
    ref = oracle_rows(kind, params, A.OVERFLOW_FREQS, rl, interp)
    got = device_rows(kind, params, A.OVERFLOW_FREQS, dtype, rl, interp)
    bad_ref = ~np.all(np.isfinite(ref), axis=1)
    bad_got = ~np.all(np.isfinite(got), axis=1)
    for i, f in enumerate(A.OVERFLOW_FREQS):
        same = np.array_equal(np.isnan(got[i]), np.isnan(ref[i])) and np.array_equal(np.isinf(got[i]), np.isinf(ref[i]))
        print(f'b=100 {dtype} {f} Hz: oracle {np.isinf(ref[i]).sum()} inf {np.isnan(ref[i]).sum()} NaN, '
              f'device {np.isinf(got[i]).sum()} inf {np.isnan(got[i]).sum()} NaN, bin masks equal: {same}')
    assert bad_ref.tolist() == [True, True, False, False]
    assert bad_got.tolist() == bad_ref.tolist()
    err = row_errors(got[~bad_ref], ref[~bad_ref], dtype)
    bound = 1e-13 if dtype == 'float64' else fp32_bound(kind, params)
    MEASURED[('morse-b100-r3 (finite rows)', dtype, 'full')] = float(err.max())
    print(f'b=100 {dtype}: finite rows worst {err.max():.3e}, bound {bound:.3e}')
    assert err.max() <= bound


# ---------------------------------------------------------------------------------------------------------
# one CWT per non-default family through the on-chip forms
# ---------------------------------------------------------------------------------------------------------
FAMILIES = [('morse', (3, 2)), ('morse', (17.5, 1)), ('morlet', (2, False)), ('morlet', (20, False))]
CWT_FORMS = [(1024, 1), (8192, 1), (1201, 1), (4096, 4)]        # (n, decim): one-pass E=16 / E=32, chirp, decimated
_REF = {}


def cwt_reference(case, n, dtype):
    """(x, ref): three white-noise signals in the compute dtype and their complex128 CWT, once per case."""
    key = (case, n, dtype)
    if key not in _REF:
        kind, params = case
        x = np.random.default_rng(5100 + n).standard_normal((3, n)).astype(dtype)
        rows = O.fft_wavelets(kind, FREQS, 1000., n / 1000., False, **A.oracle_params(kind, params))
        ref = np.stack([O.cwt_from_rows(s.astype(np.float64), rows, False) for s in x])
        x.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (x, ref)
    return _REF[key]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,decim', CWT_FORMS)
@pytest.mark.parametrize('case', FAMILIES, ids=A.set_id)
def test_cwt_of_a_non_default_family(case, n, decim, dtype):
    kind, params = case
    x, ref = cwt_reference(case, n, dtype)
    ref = ref[..., ::decim]
    p = nw.Plan(n, len(FREQS), dtype, max_batch=3, decim=decim)
    try:
        p.set_wavelet(kind, A.plan_params(kind, params), np.asarray(FREQS), L.trans_grid(n / 1000., 1000., False))
        got = p.execute(x)
        st = p.stats()
    finally:
        p.close()
    assert st['engine'] == 'fused', st
    assert got.shape == ref.shape
    err = np.max(np.abs(got - ref), axis=-1) / np.max(np.abs(ref), axis=-1)          # (signal, scale)
    tol = tol_of(n, dtype)
    s, f = np.unravel_index(int(err.argmax()), err.shape)
    MEASURED[(A.set_id(case), dtype, f'cwt n={n} decim={decim}')] = float(err.max())
    print(f'cwt {A.set_id(case)} n={n} decim={decim} {dtype} {L.KERNEL_NAMES[st["kernel"]]}: worst row '
          f'{err.max():.3e} (signal {s}, {FREQS[f]} Hz), tol {tol:.0e}')
    assert err.max() <= tol, (A.set_id(case), n, decim, dtype, float(err.max()))


def test_record_the_measured_ratios():
    """Last in the file: what the tests above measured, into the record (fp32 rows: also as a ratio to the floor).
    A run of a part of the file leaves the record as it is."""
    if len(MEASURED) != len(A.ROW_SETS) * len(DTYPES) * len(GRIDS) + len(DTYPES) * (1 + len(FAMILIES) * len(CWT_FORMS)):
        return
    lines = ['# rows: largest max_j |d| over the 40 scales in the unit of the bound (fp64: max(1, row peak), bound 1e-13;',
             '# fp32: row peak, bound 4 floor + 2^-23); cwt: largest max |d| / max |ref| over the (signal, scale) rows',
             f'{"set":<30}{"dtype":<9}{"what":<22}{"measured":>11}{"/ floor":>9}']
    floors = {A.set_id(c): A.floor_of(*c) for c in A.ROW_SETS}
    floors['morse-b100-r3 (finite rows)'] = A.floor_of(*A.OVERFLOW_SET)
    for (sid, dtype, what), v in sorted(MEASURED.items()):
        ratio = f'{v / floors[sid]:9.2f}' if dtype == 'float32' and not what.startswith('cwt') else ''
        lines.append(f'{sid:<30}{dtype:<9}{what:<22}{v:>11.3e}{ratio}')
    A.record('2. device rows (test_gpu_wavelet_rows.py::test_record_the_measured_ratios)', lines)
