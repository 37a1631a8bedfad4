"""The conditions that tests/test_gpu_fused_rows.py relies on, checked on the reference alone (no
GPU): for every (n, kind, K) of tests/fused_cases.py and both dtypes, with the rows taken from
oracle.nw_oracle's spectra cut at K,

  - the support of all three rows ends at K - 1: row_wnz's need is (K - 1) // TT + 1;
  - over the K of a size the rows run every pass-0 variant each kernel instantiates, for every
    output kind (the single-signal kernel; at fp32 with n <= 4096 also the signal-pair kernel);
  - the last bin shows: |W[K - 1] X[K - 1]| / n >= 100 TOL['float32'] max|ref row| for every
    (signal, row), so a kernel that drops the bin misses the fp32 bound a hundred times over;
  - at least 0.9 of a case's phase points have a phase_sum bound of at most 0.05.

These are conditions on the inputs: where a seed fails one, the seed changes, not the threshold."""
import numpy as np
import pytest

import fused_cases as C
from fused_variants import elems_per_thread, instantiated_variants, row_wnz, variant_of

VISIBLE = 100 * C.TOL['float32']


def test_support_lists():
    assert [len(C.supports(n)) for n in C.SIZES] == [11, 11, 11, 19, 19]
    for n in C.SIZES:
        ks = C.supports(n)
        tt = n // elems_per_thread(n)
        assert ks == sorted(set(ks)) and ks[0] == tt and ks[-1] == n and 1 not in ks
        assert n // 2 in ks and n // 2 + 1 in ks            # the Nyquist bin outside and inside
        assert set(C.pair_supports(n)) <= set(ks)


def test_reduce_path_table_covers_every_case():
    assert set(C.PARTIALS) == {(d, o) for d in C.DTYPES for o in ('power_sum', 'phase_sum')}
    assert all(v <= set(C.SIZES) for v in C.PARTIALS.values())


def test_group_filling_restated():
    c = C.shape_constants()
    assert c['min_rounds'] * c['resident'] == 2048 and c['group'] == 8
    for n, dtype in ((8192, 'float32'), (8192, 'float64'), (4096, 'float64'), (16384, 'float32')):
        base = C.group_base(n, dtype, c)
        assert C.group_filling(base, 67, 256, c) == 8       # part C's launch
        assert C.group_filling(base, 2, 256, c) == 2
    assert C.group_filling(8, 5, 3, c) == 2 and C.group_filling(8, 9, 9, c) == 2
    assert C.group_filling(8, 64, 128, c) == 4 and C.group_filling(8, 512, 256, c) == 8


def test_signals_are_flat_and_seeded():
    for n in C.SIZES:
        x = C.signals(n, 'float64')
        mag = np.abs(np.fft.fft(x, axis=-1)) / np.sqrt(n)
        assert x.shape == (C.S, n) and np.max(np.abs(mag - 1)) <= 1e-9
        assert np.array_equal(C.signals(n, 'float32'), x.astype(np.float32))
        assert 0.9 <= np.std(x) <= 1.1


def test_nyquist_signs_differ_inside_every_block():
    """The signals with other Nyquist bins: the same signals but for that bin, flat like them; the
    signs differ inside every block of 2 of the 5, and inside every block of 8 of part C's 67 from
    the block's first signal.  At K = n / 2 + 1 the Nyquist bin is the row's last, whose worth
    test_conditions_on_the_inputs asserts."""
    n = 1024
    x, y = C.signals(n, 'float64'), C.signals(n, 'float64', C.S, C.NYQUIST_ALTERNATE)
    d = np.fft.fft(y - x, axis=-1) / np.sqrt(n)
    assert np.max(np.abs(d[:, :n // 2])) <= 1e-9 and np.max(np.abs(d[:, n // 2 + 1:])) <= 1e-9
    np.testing.assert_allclose(d[:, n // 2].real, [0, 2, 0, 2, 0], atol=1e-9)
    assert all(C.NYQUIST_ALTERNATE[s] != C.NYQUIST_ALTERNATE[s + 1] for s in (0, 2))
    lead = C.nyquist_lead(67)
    assert len(lead) == 67 and all(lead[s] != lead[s - s % 8] for s in range(67) if s % 8)
    assert n // 2 + 1 in C.supports(n)


@pytest.mark.parametrize('kind', sorted(C.KIND_PARAMS))
@pytest.mark.parametrize('n', C.SIZES)
def test_conditions_on_the_inputs(n, kind):
    e = elems_per_thread(n)
    tt = n // e
    wnz = {d: set() for d in C.DTYPES}
    worst_visible, worst_share = np.inf, 1.0
    for k in C.supports(n):
        rows = C.oracle_rows(kind, n, k)
        assert np.all(rows[:, k:] == 0) and np.all(rows[:, k - 1] != 0) and np.all(np.isfinite(rows))
        assert np.all(np.ptp(rows[:, 1:k], axis=1) > 0)
        for dtype in C.DTYPES:
            for row in rows:
                w, need = row_wnz(row.astype(dtype), n, dtype)
                assert need == (k - 1) // tt + 1, (k, dtype, need)
                wnz[dtype].add(w)
            x = C.signals(n, dtype)
            ref = C.reference(x, rows.astype(dtype))
            top = C.row_max(ref)                                          # (S, F)
            spec = np.fft.fft(x.astype(np.float64), axis=-1)
            last = np.abs(rows[None, :, k - 1] * spec[:, None, k - 1]) / n
            worst_visible = min(worst_visible, float(np.min(last / top)))
            share = float(np.mean(C.phase_sum_bound(ref, 'float32') <= C.PHASE_CAP))
            worst_share = min(worst_share, share)
    print(f'{kind} n={n}: last bin at least {worst_visible:.2e} of max|ref row| (needs {VISIBLE:.0e}); '
          f'phase points under the cap: at least {worst_share:.4f}')
    assert worst_visible >= VISIBLE, 'the last bin would hide under the fp32 bound: choose another seed'
    assert worst_share >= C.PHASE_SHARE, 'too few phase points under the cap: choose another seed'
    for dtype in C.DTYPES:
        for out in C.OUTS:
            for pair in ([False, True] if C.pair_kernel(n, dtype) else [False]):
                variants = instantiated_variants(n, dtype, out, pair)
                hit = {variant_of(w, variants) for w in wnz[dtype]}
                assert hit == variants, (dtype, out, pair, sorted(hit), sorted(variants))
