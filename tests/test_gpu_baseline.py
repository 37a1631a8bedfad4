"""GPU parity of nw_baseline (k_bl_partial, k_bl_final, k_bl_apply; Baseline of ninwavelets_amd/baseline.py) against
oracle.nw_oracle.baseline, past the goldens (at most 262 144 elements with an 81 920-element baseline, float64 and
float32 host arrays, 2-D).

The grid-stride case is sized past one sweep of both grids: k_bl_partial runs at most 1024 blocks of 256 threads, so
its loop takes a second step only for a slice above 262 144 elements; k_bl_apply at most 8192 blocks of 256, so above
2 097 152 elements.  (131, 16381) with rows [4, 24) gives a slice of 327 620 and a count of 2 145 911, neither a
multiple of 256.  The real use, Baseline(power(F = 256, N = 16384)), has 4 M elements.

Bounds (test_gpu_parity.py's test_baseline_against_reference): 1e-13 of max |ref| for float64 data; 2e-6 for float32
data, against numpy's float32 result (numpy reduces the mean pairwise in float32, the device in fp64 and rounds; on
the grid-stride input numpy's float32 result is itself within 8e-7 of the float64 evaluation, which the test prints).
Where numpy gives inf or NaN (zero basemean, zero std, log10 of a negative) the masks must be equal and the finite
values within the bound."""
import warnings

import numpy as np
import pytest

import aux_cases as A
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402

TOL = {'float64': 1e-13, 'float32': 2e-6}
DTYPES = ['float64', 'float32']
MEASURED = {}


def rel_err(got, ref):
    return np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))) / max(np.max(np.abs(ref)), 1e-300)


def oracle(wave, sfreq, start, stop, op):
    with np.errstate(all='ignore'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')              # numpy's "Mean of empty slice"
            return O.baseline(wave, sfreq, start, stop, op)


# ---------------------------------------------------------------------------------------------------------
# both grid-stride loops
# ---------------------------------------------------------------------------------------------------------
BIG = (131, 16381)
BIG_ARGS = (1.0, 4., 24.)
_BIG = {}


def big(dtype):
    """(wave, {op: numpy's result in the data's dtype}, {op: the float64 evaluation}), once per dtype."""
    if dtype not in _BIG:
        w64 = np.random.default_rng(41).uniform(0.5, 2.0, BIG)
        w = w64.astype(dtype)
        ref = {op: oracle(w, *BIG_ARGS, op) for op in O.BASELINE_OPS}
        ref64 = {op: oracle(w.astype(np.float64), *BIG_ARGS, op) for op in O.BASELINE_OPS}
        for a in [w, *ref.values(), *ref64.values()]:
            a.setflags(write=False)
        _BIG[dtype] = (w, ref, ref64)
    return _BIG[dtype]


def test_the_case_is_past_both_grid_sweeps():
    w, _, _ = big('float64')
    b = nw.Baseline(w, *BIG_ARGS)
    assert b.baseline.size == 327620 > 1024 * 256 and b.baseline.size % 256
    assert w.size == 2145911 > 8192 * 256 and w.size % 256


@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_stride_case(dtype, where):
    torch = pytest.importorskip('torch')
    w, ref, ref64 = big(dtype)
    x = torch.from_numpy(w.copy()).cuda() if where == 'device' else w
    b = nw.Baseline(x, *BIG_ARGS)
    part = w[4:24].astype(np.float64)
    for op in O.BASELINE_OPS:
        got = getattr(b, op)()
        if where == 'device':
            assert got.is_cuda and got.dtype == x.dtype and got.shape == x.shape
            got = got.cpu().numpy()
        assert got.dtype == ref[op].dtype == np.dtype(dtype) and got.shape == ref[op].shape, op
        err, err64 = rel_err(got, ref[op]), rel_err(got, ref64[op])
        MEASURED[(dtype, where, op)] = (err, err64, rel_err(ref[op], ref64[op]))
        print(f'baseline {dtype} {where} {op}: {err:.2e} of max|ref| (bound {TOL[dtype]:.0e}); against the float64 '
              f'evaluation {err64:.2e}, numpy itself {rel_err(ref[op], ref64[op]):.2e}')
        assert err <= TOL[dtype], (dtype, where, op, err)
    mean, std = b._stats
    if dtype == 'float64':
        assert abs(b.basemean - part.mean()) <= 1e-13 * abs(part.mean())
        assert abs(std - part.std()) <= 1e-13 * part.std()
    else:       # the statistics are reduced in fp64 from the float32 data
        assert abs(mean - part.mean()) <= 1e-13 * abs(part.mean()) and abs(std - part.std()) <= 1e-13 * part.std()


def test_record_the_measured_errors():
    """After test_grid_stride_case: its figures into the record.  A run of a part of the file leaves it as it is."""
    if len(MEASURED) != len(DTYPES) * 2 * len(O.BASELINE_OPS):
        return
    lines = ['# Baseline(uniform(0.5, 2) (131, 16381), 1.0, 4., 24.): slice 327 620, count 2 145 911 (both grid-stride loops)',
             '# max |got - ref| / max |ref|: against numpy in the data\'s dtype (the bound: 1e-13 float64, 2e-6 float32),',
             '# against the float64 evaluation of the same data, and numpy\'s own result against that evaluation',
             f'{"dtype":<9}{"arrays":<8}{"op":<9}{"vs numpy":>11}{"vs float64":>12}{"numpy vs float64":>18}']
    for (dtype, where, op), (e, e64, en) in sorted(MEASURED.items()):
        lines.append(f'{dtype:<9}{where:<8}{op:<9}{e:>11.2e}{e64:>12.2e}{en:>18.2e}')
    A.record('3. baseline (test_gpu_baseline.py::test_record_the_measured_errors)', lines)


# ---------------------------------------------------------------------------------------------------------
# shapes and slices
# ---------------------------------------------------------------------------------------------------------
def check(wave, sfreq, start, stop, ops=O.BASELINE_OPS, what=''):
    """Every op of Baseline(wave, ...) against the oracle: dtype, shape, equal NaN / inf masks, finite values within
    the bound of the result's dtype."""
    b = nw.Baseline(wave, sfreq, start, stop)
    for op in ops:
        ref = oracle(wave, sfreq, start, stop, op)
        got = getattr(b, op)()
        assert got.dtype == ref.dtype and got.shape == ref.shape, (what, op, got.dtype, ref.dtype)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, op, 'NaN mask')
        assert np.array_equal(np.isposinf(got), np.isposinf(ref)), (what, op, '+inf mask')
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (what, op, '-inf mask')
        ok = np.isfinite(ref)
        if ok.any():
            err = rel_err(got[ok], ref[ok])
            assert err <= TOL[str(ref.dtype)], (what, op, err)
    return b


def test_shapes():
    rng = np.random.default_rng(42)
    check(rng.uniform(0.5, 2.0, 500).astype(np.float32), 10., 3., 21.5, what='1-D float32')
    check(rng.uniform(0.5, 2.0, (3, 5, 700)), 1., 1., 3., what='3-D')
    check(rng.uniform(0.5, 2.0, (3, 5, 700)).astype(np.float32), 1., 0., 2., what='3-D float32')
    wide = rng.uniform(0.5, 2.0, (40, 600))
    view = wide[::2, 1::3]
    assert not view.flags.c_contiguous
    check(view, 1., 2., 11., what='non-contiguous view')
    check(wide.T, 10., 1., 30., what='transposed view')
    ints = rng.integers(1, 50, (40, 300))
    b = check(ints, 1., 5., 25., what='integers')
    assert b.mean().dtype == np.float64


@pytest.mark.parametrize('dtype', DTYPES)
def test_slices(dtype):
    w = np.random.default_rng(43).uniform(0.5, 2.0, (64, 515)).astype(dtype)
    for start, stop, rows in ((-2.0, 6.0, (44, 60)), (0.5, -1.0, (5, 54)), (3.0, 100.0, (30, 64)), (0.0, 6.4, (0, 64)),
                              (-100.0, 1.0, (0, 10))):
        b = check(w, 10., start, stop, what=(dtype, start, stop))
        assert b.baseline.shape == w[rows[0]:rows[1]].shape, (start, stop)
    for start, stop in ((10.0, 12.0), (3.0, 1.0), (6.4, 6.4)):                    # empty: every op all-NaN
        b = check(w, 10., start, stop, what=(dtype, start, stop))
        assert b.baseline.size == 0
        for op in O.BASELINE_OPS:
            assert np.all(np.isnan(getattr(b, op)())), (start, stop, op)
        assert np.isnan(b.basemean)


@pytest.mark.parametrize('dtype', DTYPES)
def test_numpys_special_values(dtype):
    rng = np.random.default_rng(44)
    w = rng.uniform(0.5, 2.0, (48, 301))
    w[::7, ::5] = 0.                         # zeros outside and inside the baseline rows too
    # baseline rows all zero: basemean 0, so ratio / percent / log divide by 0 (x / 0 = inf, 0 / 0 = NaN)
    z = w.copy()
    z[8:16] = 0.
    check(z.astype(dtype), 1., 8., 16., ops=('ratio', 'percent', 'log'), what='zero basemean')
    # constant baseline rows: std exactly 0 (1.5 n is exact), so zscore / zlog divide by 0
    c = w.copy()
    c[8:16] = 1.5
    b = check(c.astype(dtype), 1., 8., 16., ops=('zscore', 'zlog'), what='zero std')
    assert b._stats == (1.5, 0.0)
    # negative entries: log10 of a negative is NaN, of zero -inf
    m = w.copy()
    m[rng.uniform(size=m.shape) < 0.1] *= -1.
    ref = oracle(m.astype(dtype), 1., 8., 16., 'log')
    assert np.isnan(ref).any() and np.isneginf(ref).any() and np.isfinite(ref).any()
    check(m.astype(dtype), 1., 8., 16., ops=('log', 'zlog'), what='negative entries')


def test_special_values_on_device_tensors():
    """The same masks from torch tensors (no host staging): zero basemean under ratio, float32 and float64."""
    torch = pytest.importorskip('torch')
    for dtype in DTYPES:
        w = np.random.default_rng(45).uniform(0.5, 2.0, (16, 130)).astype(dtype)
        w[2:5] = 0.
        w[9, ::3] = 0.
        ref = oracle(w, 1., 2., 5., 'ratio')
        got = nw.Baseline(torch.from_numpy(w).cuda(), 1., 2., 5.).ratio()
        assert got.is_cuda
        got = got.cpu().numpy()
        assert got.dtype == ref.dtype
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
        assert np.isnan(ref).any() and np.isposinf(ref).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_object_many_calls(dtype):
    """Two ops on one Baseline object, and basemean read before any op, agree with fresh objects bit for bit."""
    w = np.random.default_rng(46).uniform(0.5, 2.0, (37, 1001)).astype(dtype)
    args = (1., 3., 17.)
    one = nw.Baseline(w, *args)
    mean_first = one.basemean                             # before any op
    a, c, a2 = one.zlog(), one.percent(), one.zlog()
    np.testing.assert_array_equal(a, nw.Baseline(w, *args).zlog())
    np.testing.assert_array_equal(c, nw.Baseline(w, *args).percent())
    np.testing.assert_array_equal(a, a2)
    fresh = nw.Baseline(w, *args)
    fresh.ratio()
    assert mean_first == fresh.basemean == one.basemean
    assert abs(mean_first - w[3:17].astype(np.float64).mean()) <= 1e-13 * mean_first
