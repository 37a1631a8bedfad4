"""The chirp-z algorithm of nw_chirp.hip as a numpy model in complex128, and the sensitivity of
the inputs tests/test_gpu_chirp_rows.py uses to one bin of wrap (no GPU).

chirp_model(x, row, M) is the kernel's arithmetic at transform length M: a = W X c zero-padded to
M, b the chirp of chirp_bhat_kernel at length M (lags -(M - n) .. n - 1), y = c IDFT(FFT a FFT b).
A row of support K is wrap-free at M iff M >= n + K - 1 (tests/chirp_variants.py chirp_class).  At
the last such K the model equals the oracle to 1e-12; one bin past it exactly one lag is
aliased, and how large the error is depends on the phase difference of the two colliding chirp
terms, i.e. on n: at n = M / 2 + 1 it is invisible (b(-j) = b(j)), at n = M / 2 + 2 it is below
the fp32 bound.  The GPU test's lengths n = M / 2 + WRAP_DELTA are held here to an error of at
least 10 x that bound (2e-4 of the row's maximum) with white-noise signals and hard-edged rows, so
a class or wrap off-by-one in the kernel, its support scan or chirp_class fails there."""
import numpy as np
import pytest

import chirp_variants as V
from oracle import nw_oracle as O

SENSITIVE = 10 * 2e-5          # 10 x the fp32 bound of tests/test_gpu_chirp_rows.py


def chirp_model(x, row, m):
    """(n,) complex128: the chirp-z transform of nw_chirp.hip at length ``m`` for the signal x
    (n,) and the W row (n,) as pad_to leaves it (the 1 / n of the inverse transform applied here)."""
    n = x.shape[0]
    k = np.arange(n)
    c = np.exp(1j * np.pi * ((k * k) % (2 * n)) / n)
    a = np.zeros(m, dtype=np.complex128)
    a[:n] = row / n * np.fft.fft(x.astype(np.float64)) * c
    p = np.arange(m)
    j = np.where(p < n, p, p - m)                       # chirp_bhat_kernel's lag of slot p
    b = np.where(j > -n, np.exp(-1j * np.pi * ((j * j) % (2 * n)) / n), 0.0)
    return c * np.fft.ifft(np.fft.fft(a) * np.fft.fft(b))[:n]


def rel_err(got, ref):
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def case_rows(m, k):
    """The table row and the Shannon row of support k at the wrap length of M, as the GPU test builds
    them."""
    n, _ = V.wrap_case(m)
    table = V.hard_rows([k], n, 11 + m)[0]
    shannon = V.shannon_row(V.shannon_delta(k), n)
    assert V.table_support(table) == k and V.shannon_support(V.shannon_delta(k), n) == k
    return n, {'table': table, 'shannon': shannon.astype(np.complex128)}


CASES = [('float32', m) for m in V.CLASSES] + [('float64', m) for m in V.CLASSES[:4]]


@pytest.mark.parametrize('dtype,m', CASES)
def test_model_is_exact_in_the_class_chirp_class_gives(dtype, m):
    """K = M - n + 1 is the last support chirp_class puts into M, K + 1 goes to 2M (or off chip at
    the top); at the M it names the model equals cwt_from_rows within 1e-12 for both rows.  (With
    chirp_class admitting one bin more, the K + 1 rows run at M and miss by >= 1e-3.)"""
    n, kb = V.wrap_case(m)
    assert n + kb - 1 == m and 2 * (kb + 1) <= m
    top = m == V.chirp_mmax(dtype)
    x = V.noise(1, n, 21 + m, np.float64)[0]
    for k in (kb, kb + 1):
        mk = V.chirp_class(n, k, dtype)
        if mk < 0:
            continue
        for name, row in case_rows(m, k)[1].items():
            ref = O.cwt_from_rows(x, [row], False)[0]
            err = rel_err(chirp_model(x, row, mk), ref)
            print(f'{dtype} M={m} n={n} K={k} at M={mk} {name}: {err:.2e}')
            assert err <= 1e-12, (name, k, mk, err)
    assert V.chirp_class(n, kb, dtype) == m
    assert V.chirp_class(n, kb + 1, dtype) == (-1 if top else 2 * m)


@pytest.mark.parametrize('m', V.CLASSES)
def test_one_bin_of_wrap_shows_at_the_test_lengths(m):
    """The same M with K + 1: some output sample is off by at least SENSITIVE of the row's maximum,
    for the table row and for the Shannon row."""
    n, kb = V.wrap_case(m)
    x = V.noise(1, n, 21 + m, np.float64)[0]
    for name, row in case_rows(m, kb + 1)[1].items():
        ref = O.cwt_from_rows(x, [row], False)[0]
        err = rel_err(chirp_model(x, row, m), ref)
        print(f'M={m} n={n} K+1={kb + 1} {name}: {err:.2e}')
        assert err >= SENSITIVE, (name, err)


@pytest.mark.parametrize('dtype,m', CASES)
def test_lengths_reach_the_classes_the_gpu_test_claims(dtype, m):
    """n = M / 2 + 1: every K in 0 .. M / 2 falls in class M (both corners, 2K == M and
    n + K - 1 == M, at K = M / 2) and K = n in 2M, off chip at the top, where the length is tentative.
    n = M / 2 - 1: every K in 3 .. M / 2 - 1 falls in class M and the length is not tentative."""
    top = m == V.chirp_mmax(dtype)
    n = m // 2 + 1
    assert {V.chirp_class(n, k, dtype) for k in range(m // 2 + 1)} == {m}
    assert n + m // 2 - 1 == m
    assert V.chirp_class(n, n, dtype) == (-1 if top else 2 * m)
    assert V.chirp_possible(n, dtype) and V.chirp_supported(n, dtype) == (not top)
    n = m // 2 - 1
    assert {V.chirp_class(n, k, dtype) for k in range(3, m // 2)} == {m}
    assert V.chirp_supported(n, dtype)
