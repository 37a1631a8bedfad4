"""GPU parity of the time-domain wavelets, make_wavelet(s) (nw_make_wavelets: k_wavelet_spectra + one rocFFT inverse
per row length + k_wavelet_pack for Morse / Shannon, k_wavelet_time for Morlet / MexicanHat / Haar), against
oracle.nw_oracle.make_wavelets over the sweep of tests/aux_cases.py: sampling rates and lengths that give an odd
spectrum length m in the conj-flip slice (sfreq 999: m = 999, also a non-smooth rocFFT length, 27 x 37; 0.301 s:
m = 301), rows of two lengths in one call (the by-length grouping, the scratch offsets, one plan per length) and
every stock kind with non-default parameters.  test_aux_cases_cpu.py asserts on the oracle that the sweep has them.

Bound: the ragged shapes and the dtype equal the oracle's; each row within 1e-13 of its peak
(test_gpu_parity.py's test_make_wavelets_against_reference)."""
import numpy as np
import pytest

import aux_cases as A

pytestmark = pytest.mark.gpu

TOL = 1e-13


def assert_rows(got, ref, what):
    assert [r.shape for r in got] == [r.shape for r in ref], what
    worst = 0.0
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == r.dtype, (what, i, g.dtype, r.dtype)
        err = np.max(np.abs(g - r)) / max(1e-300, np.max(np.abs(r)))
        worst = max(worst, err)
        assert err <= TOL, (what, i, len(r), err)
    return worst


@pytest.mark.parametrize('sfreq,rwl', A.SWEEP)
@pytest.mark.parametrize('name', list(A.SWEEP_KINDS))
def test_make_wavelets_over_the_sweep(name, sfreq, rwl):
    w = A.sweep_wavelet(name, sfreq, rwl)
    assert w._device_wavelet_spec() is not None
    ref = A.sweep_oracle(name, A.SWEEP_FREQS, sfreq, rwl)
    got = w.make_wavelets(A.SWEEP_FREQS)
    worst = assert_rows(got, ref, (name, sfreq, rwl))
    print(f'{name} sfreq={sfreq} rwl={rwl}: lengths {sorted({len(r) for r in ref})}, worst {worst:.2e} of a row peak')
    # one row on its own is the batch's row bit for bit: a frequency whose length differs from its neighbours'
    # where there is one, and one whose length does not
    lens = [len(r) for r in ref]
    odd_one = [i for i in range(1, len(lens) - 1) if lens[i] != lens[i - 1] or lens[i] != lens[i + 1]]
    plain = [i for i in range(1, len(lens) - 1) if lens[i] == lens[i - 1] == lens[i + 1]]
    for i in odd_one[:1] + plain[:1]:
        np.testing.assert_array_equal(w.make_wavelet(A.SWEEP_FREQS[i]), got[i])


@pytest.mark.parametrize('name', ['morse', 'shannon', 'morlet_s5', 'mexican_hat'])
def test_order_of_the_frequencies_does_not_matter(name):
    """sfreq 999 (Reverse kinds: lengths 998 and 1000 from m = 999 and 1000) and 1000 (1000 and 1001 for the time
    kinds): the scratch offsets are assigned per length group, so a descending or shuffled list gives the same rows."""
    sfreq = 999 if name in ('morse', 'shannon') else 1000
    w = A.sweep_wavelet(name, sfreq, 1)
    asc = w.make_wavelets(A.SWEEP_FREQS)
    assert len({len(r) for r in asc}) == 2
    for order in (np.arange(len(asc))[::-1], np.random.default_rng(7).permutation(len(asc))):
        rows = w.make_wavelets([A.SWEEP_FREQS[i] for i in order])
        for pos, i in enumerate(order):
            np.testing.assert_array_equal(rows[pos], asc[i])


@pytest.mark.parametrize('name', list(A.SWEEP_KINDS))
def test_zero_and_negative_frequencies(name):
    w = A.sweep_wavelet(name, 1000, 1)
    with pytest.raises(ZeroDivisionError):
        w.make_wavelets([3., 0., 7.])
    with pytest.raises(ZeroDivisionError):
        w.make_wavelet(0)
    freqs = [-3.3, 7., -40.]
    with np.errstate(all='ignore'):
        ref = A.sweep_oracle(name, freqs, 1000, 1)
    got = w.make_wavelets(freqs)
    assert [r.shape for r in got] == [r.shape for r in ref]
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r))
        ok = np.isfinite(r)
        if ok.any():
            assert np.max(np.abs(g[ok] - r[ok])) <= TOL * max(1e-300, np.max(np.abs(r[ok])))
