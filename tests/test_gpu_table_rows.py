"""GPU parity of the complex-row instantiations of the one-pass kernels:
nw_fused_kernel<T, N, E, OUT, REALW = false> (nw_fused.hip), which runs NW_TABLE wavelets (user
plugins, the device-built MexicanHat / Haar tables) with its own W table and support kernels, no
X LDS-DMA, no W registers kept at E = 32 and a complex multiply in pass 0.

Every case attaches a user table to a plan (nw.Plan.set_wavelet('table', ...)) at a power-of-two
n = 1024 .. 16384 and compares with oracle.nw_oracle.cwt_from_rows in complex128 on the exact
rows handed to the plan (|.| and |.|^2 taken from it).  Tolerance, per signal: the parity
contract of tests/test_gpu_parity.py, max|got - ref| <= 1e-12 (fp64) / 1e-5 (fp32) of max|ref|,
doubled for power.  Every run asserts the fused engine and the kernel nw_fused_kernel.

Signals are white noise; a row is complex normal on its support, exactly zero elsewhere, divided
by the square root of its support length, so every row of a signal has the same expected output
energy.  So that a wrong row cannot hide under the per-signal maximum, every (signal, row) must
reach 0.25 of the signal's max|ref|: asserted on the reference alone before the GPU result is
looked at (visible())."""
import numpy as np
import pytest

from fused_variants import elems_per_thread, instantiated_variants, row_wnz, variant_of
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

TOL = {'float64': 1e-12, 'float32': 1e-5}
VISIBLE = 0.25
SIZES = [1024, 2048, 4096, 8192, 16384]


def noise(S, n, seed, dtype):
    """White noise in the compute dtype (the reference sees the same rounded values)."""
    return np.random.default_rng(seed).standard_normal((S, n)).astype(dtype)


def make_rows(supports, length, seed):
    """(len(supports), length) complex128: row i is complex normal on [0, supports[i]) / sqrt(supports[i]),
    exactly zero from there on."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((len(supports), length), dtype=np.complex128)
    for i, k in enumerate(supports):
        if k:
            tab[i, :k] = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.sqrt(k)
    return tab


def reference(x, table, row_len, interpolate=False):
    """(S, F, n) complex128: cwt_from_rows on the rows as the plan holds them (row i is its first
    row_len[i] bins: cropped to n or centre-padded, base.py:75-82)."""
    rows = [table[i, :m] for i, m in enumerate(row_len)]
    return np.stack([O.cwt_from_rows(xi.astype(np.float64), rows, interpolate) for xi in x])


def as_kind(c, out):
    return c if out == 'cwt' else np.abs(c) if out == 'abs' else np.abs(c) ** 2


def visible(want, rows):
    """The 0.25 condition on the reference: each of ``rows`` reaches VISIBLE of its signal's max."""
    top = np.max(np.abs(want), axis=(1, 2))
    per_row = np.max(np.abs(want), axis=2)
    worst = np.min(per_row[:, rows] / top[:, None])
    assert worst >= VISIBLE, f'a row reaches only {worst:.3f} of its signal\'s max|ref|: choose another seed'


def run_table(n, dtype, table, row_len, x, out, max_batch, interpolate=False):
    F, lf = table.shape
    p = nw.Plan(n, F, dtype, max_batch=max_batch, interpolate=interpolate)
    try:
        p.set_wavelet('table', [], np.arange(1., F + 1), L.nw_grid(1.0, lf, lf), table=table, row_len=row_len)
        got = p.execute(x, out_kind=out)
        st = p.stats()
    finally:
        p.close()
    assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_kernel', st
    return got


def check(got, want, dtype, out, what, rows=slice(None)):
    """Per signal, over ``rows``: max|got - want| <= tol x max|want|."""
    assert got.shape == want.shape, (got.shape, want.shape)
    t = TOL[dtype] * (2 if out == 'power' else 1)
    g, w = got[:, rows], want[:, rows]
    err = np.max(np.abs(g - w), axis=(1, 2)) / np.max(np.abs(w), axis=(1, 2))
    print(f'{what}: rel err per signal {np.array2string(err, precision=3)} (tol {t:.0e})')
    assert np.all(err <= t), (what, err)


# ------------------------------------------------------------------ 1. every pass-0 variant
def variant_supports(n, dtype, out):
    """One hard support [0, K) per instantiated pass-0 variant NZ, K = (NZ - 0.5) n / E: need == NZ,
    the middle of its bucket; for the variant 4 also need = 1 and need = 3."""
    tt = n // elems_per_thread(n)
    needs = [1, 3] + sorted(instantiated_variants(n, dtype, out, pair=False))
    return [tt // 2 if nz == 1 else (2 * nz - 1) * tt // 2 for nz in needs], needs


_variant_ref = {}


def variant_case(n, dtype, out):
    supports, needs = variant_supports(n, dtype, out)
    key = (n, dtype, tuple(supports))
    if key not in _variant_ref:
        table = make_rows(supports, n, 100 + n)
        x = noise(3, n, 200 + n, dtype)
        _variant_ref[key] = (x, table, reference(x, table, [n] * len(supports)))
    return _variant_ref[key] + (needs,)


@pytest.mark.parametrize('out', ['cwt', 'abs', 'power'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n', SIZES)
def test_table_every_pass0_variant(n, dtype, out):
    """S = 3 in one chunk; one row per pruned pass-0 variant the kernel instantiates (F = 5 .. 9,
    no multiple of the 8-scale tile at E = 32).  Which variant a row takes is asserted from the
    table itself with the rule of tests/fused_variants.py: a miss fails."""
    x, table, ref, needs = variant_case(n, dtype, out)
    variants = instantiated_variants(n, dtype, out, pair=False)
    got_needs = [row_wnz(row, n, dtype)[1] for row in table]
    assert got_needs == needs, (got_needs, needs)
    hit = {variant_of(row_wnz(row, n, dtype)[0], variants) for row in table}
    assert hit == variants, f'pass-0 variants hit {sorted(hit)} != instantiated {sorted(variants)}'
    assert 5 <= len(table) <= 9
    want = as_kind(ref, out)
    visible(want, np.arange(len(table)))
    got = run_table(n, dtype, table, None, x, out, max_batch=3)
    check(got, want, dtype, out, f'variants n={n} {dtype} {out}')


# ------------------------------------------------------------------ 2. row geometry
_geometry_ref = {}


def geometry_case(n, dtype):
    if (n, dtype) not in _geometry_ref:
        row_len = [n + 64, n, n - 1, n - 8, 1000, 1, 0]
        table = make_rows(row_len, n + 64, 300 + n)
        x = noise(3, n, 400 + n, dtype)
        _geometry_ref[n, dtype] = (x, table, row_len, reference(x, table, row_len))
    return _geometry_ref[n, dtype]


@pytest.mark.parametrize('out', ['cwt', 'power'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n', [4096, 16384])
def test_table_ragged_cropped_and_empty_rows(n, dtype, out):
    """len_full = n + 64: a cropped row, an exact one, three centre-padded ones (odd and even
    padding), a one-bin row and an empty row (pad_to, base.py:75-82).  The one-bin row is held
    to its own max|ref|; the empty row's output is exactly zero."""
    x, table, row_len, ref = geometry_case(n, dtype)
    want = as_kind(ref, out)
    full = np.arange(5)
    visible(want, full)
    assert np.all(want[:, 6] == 0) and np.all(np.max(np.abs(want[:, 5]), axis=-1) > 0)
    got = run_table(n, dtype, table, row_len, x, out, max_batch=3)
    assert got.shape == want.shape
    check(got, want, dtype, out, f'geometry n={n} {dtype} {out}', rows=full)
    check(got, want, dtype, out, f'one-bin row n={n} {dtype} {out}', rows=slice(5, 6))
    assert np.all(got[:, 6] == 0), 'the empty row must give exact zeros'


# ------------------------------------------------------------------ 3. interpolate
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('n', [2048, 8192, 16384])
def test_table_interpolate(n, dtype):
    """NW_INTERPOLATE zeroes the spectrum from bin n / 2 up (interpolate_alias, base.py:107-123,
    400-401); the rows have full support, so a kernel ignoring xlim is O(1) wrong."""
    F = 5
    table = make_rows([n] * F, n, 500 + n)
    x = noise(3, n, 600 + n, dtype)
    ref = reference(x, table, [n] * F, interpolate=True)
    plain = reference(x, table, [n] * F, interpolate=False)
    assert np.max(np.abs(ref - plain)) >= 0.25 * np.max(np.abs(ref))     # the mask matters here
    visible(ref, np.arange(F))
    got = run_table(n, dtype, table, None, x, 'cwt', max_batch=3, interpolate=True)
    check(got, ref, dtype, 'cwt', f'interpolate n={n} {dtype}')


# ------------------------------------------------------------------ 4. several groups and chunks
@pytest.mark.parametrize('out', ['cwt', 'abs'])
@pytest.mark.parametrize('n,dtype', [(4096, 'float32'), (16384, 'float64')])
def test_table_many_signals(n, dtype, out):
    """S = 19 as chunks of 8, 8, 3 and as one launch over several signal groups: both against
    the reference, and bit for bit equal to each other (a row's output depends on its W row and
    its signal only)."""
    S, F = 19, 6
    table = make_rows([n] * F, n, 700 + n)
    x = noise(S, n, 800 + n, dtype)
    want = as_kind(reference(x, table, [n] * F), out)
    visible(want, np.arange(F))
    chunks = run_table(n, dtype, table, None, x, out, max_batch=8)
    check(chunks, want, dtype, out, f'many signals n={n} {dtype} {out} max_batch=8')
    one = run_table(n, dtype, table, None, x, out, max_batch=S)
    check(one, want, dtype, out, f'many signals n={n} {dtype} {out} max_batch={S}')
    np.testing.assert_array_equal(chunks, one)


# ------------------------------------------------------------------ 5. epoch reductions
@pytest.mark.parametrize('n,dtype', [(4096, 'float32'), (8192, 'float64')])
def test_table_epoch_reductions_one_pass(n, dtype):
    """Epoch reductions (mneutils.py:42-71) of table rows on the one-pass form: the per-signal
    chunk path (fused_psum_supported is false for NW_TABLE), S = 11 in chunks of 4, 4, 3.  As
    test_chirp_table_rows_epoch_reductions: power_mean and ITC against the same plan's
    materialised cwt and power_mean against the reference; as
    test_epoch_reductions_match_materialised: the sum kinds are the un-normalised accumulators
    (one rounding to the compute dtype)."""
    S, F = 11, 6
    f64 = dtype == 'float64'
    table = make_rows([n] * F, n, 900 + n)
    x = noise(S, n, 1000 + n, dtype)
    ref = reference(x, table, [n] * F)
    visible(ref, np.arange(F))
    p = nw.Plan(n, F, dtype, max_batch=4)
    try:
        p.set_wavelet('table', [], np.arange(1., F + 1), L.nw_grid(1.0, n, n), table=table)
        res = {}
        for kind in ('power_mean', 'itc', 'power_sum', 'phase_sum', 'cwt'):
            res[kind] = p.execute(x, out_kind=kind)
            st = p.stats()
            assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_kernel', (kind, st)
    finally:
        p.close()
    pm, itc, ps, ph = res['power_mean'], res['itc'], res['power_sum'], res['phase_sum']
    c = res['cwt'].astype(np.complex128)
    assert pm.shape == (F, n) and pm.dtype == np.dtype(dtype) and itc.dtype == np.dtype(dtype)
    assert ps.dtype == np.float64 and ph.dtype == np.complex128
    np.testing.assert_allclose(pm, np.mean(np.abs(c) ** 2, axis=0), rtol=1e-12 if f64 else 1e-5)
    d_itc = np.max(np.abs(itc - np.abs(np.mean(c / np.abs(c), axis=0))))
    want_pm = np.mean(np.abs(ref) ** 2, axis=0)
    e_pm = np.max(np.abs(pm - want_pm)) / np.max(np.abs(want_pm))
    one = 1e-15 if f64 else 1.2e-7                    # one rounding to the compute dtype
    e_ps = np.max(np.abs(pm - ps / S)) / np.max(np.abs(ps / S))
    e_ph = np.max(np.abs(itc - np.abs(ph) / S))
    print(f'reductions n={n} {dtype}: itc vs cwt {d_itc:.3e}, power_mean vs ref {e_pm:.3e}, '
          f'power_sum/S {e_ps:.3e}, |phase_sum|/S {e_ph:.3e}')
    assert d_itc <= (1e-12 if f64 else 1e-5)
    assert e_pm <= 2 * TOL[dtype]
    assert e_ps <= one and e_ph <= one
