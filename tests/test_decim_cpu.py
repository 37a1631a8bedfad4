"""Time decimation (decim) without a GPU: the host-only support table of the C ABI, the argument
checks of the class API, and the folding identity the decimated kernel (nw_decim.hip) rests on:

    ifft(Z)[::d][m] = (1/N) sum_{k' < ND} ( sum_{j < d} Z[k' + j ND] ) e^{2 pi i k' m / ND},  ND = N / d

checked in numpy on the oracle's rows, with the folds read as the kernel reads them: X from the
R2C half spectrum (X[k] below N/2, conj(X[N - k]) from N/2 up) and only the folds a row's support
reaches."""
import numpy as np
import pytest

from fused_variants import decim_rule as rule
from oracle import nw_oracle as O

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L


def test_decim_supported_table():
    sizes = [512 << i for i in range(7)] + [1000, 3000, 4097, 6144, 12288, 16383, 16385]
    assert sizes[0] == 512 and sizes[6] == 32768
    for dtype in (L.NW_F32, L.NW_F64):
        pairs = []
        for n in sizes:
            for decim in range(1, 33):
                got = L.decim_supported(n, dtype, decim)
                assert got == rule(n, decim), (n, dtype, decim, got)
                if got:
                    pairs.append((n, decim))
        assert len(pairs) == 10, pairs
    assert not L.decim_supported(4096, 7, 2)          # not a compute dtype
    assert not L.decim_supported(4096, L.NW_F32, 0) and not L.decim_supported(4096, L.NW_F32, -2)


@pytest.mark.parametrize('decim', [0, -2, 2.5])
def test_bad_decim_is_a_value_error_before_any_device_work(decim):
    """No device is touched: the check comes before the cache build and the plan."""
    x = np.zeros(4096)
    freqs = [1., 2., 3.]
    w = nw.Morse(1000)
    for call in (lambda: w.cwt(x, freqs, decim=decim), lambda: w.power(x, freqs, decim=decim),
                 lambda: w.abs(x, freqs, decim=decim), lambda: w.cwt_batch(x[None], freqs, decim=decim),
                 lambda: w.cwt_batch(x[None], freqs, out='power_mean', decim=decim)):
        with pytest.raises(ValueError, match='decim'):
            call()
    assert w._cache is None and not w._plans


def folded_rows(W, x, d, support=None):
    """ifft(W * fft(x))[:, ::d] the kernel's way: per row the folds j < nfold of the product, X
    taken from the half spectrum, then one ND-point inverse transform."""
    F, N = W.shape
    nd = N // d
    Xh = np.fft.rfft(x)                                   # N/2 + 1 bins
    kp = np.arange(nd)
    out = np.empty((F, nd), dtype=np.complex128)
    for f in range(F):
        reach = N if support is None else support[f]      # bins >= reach are zero
        nfold = max(1, min(d, -(-reach // nd)))
        acc = np.zeros(nd, dtype=np.complex128)
        for j in range(nfold):
            k = kp + j * nd
            if (j + 1) * nd <= N // 2:
                X = Xh[k]
            else:
                assert j * nd >= N // 2                  # a fold lies wholly on one side
                X = np.conj(Xh[N - k])
            acc += W[f, k] * X
        out[f] = np.fft.ifft(acc) / d                     # (1/N) sum = ifft_ND / d
    return out


@pytest.mark.parametrize('n,decim', [(2048, 2), (4096, 4), (16384, 16), (16384, 2)])
def test_folding_identity_morse_rows(n, decim):
    rng = np.random.default_rng(n + decim)
    x = rng.standard_normal(n)
    freqs = [1., 7., 40., 120., 250., 330., 420., 470., 499.]
    rows = O.fft_wavelets('morse', freqs, 1000., n / 1000., False)
    W = np.array([O.pad_to(r, n) for r in rows]) / 1.0
    want = O.cwt_from_rows(x, rows, False)[:, ::decim]
    # the support as the engine finds it: the last bin above 2^-72 of the row's max
    sup = [int(np.nonzero(np.abs(r) > 2.0 ** -72 * np.abs(r).max())[0][-1]) + 1 for r in W]
    assert min(sup) <= n // decim < max(sup)              # one fold for some rows, several for others
    got = folded_rows(W, x, decim, sup)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f'morse n={n} decim={decim}: {err:.2e}')
    assert err <= 1e-13                                   # fp64 FFT rounding is ~log2(n) eps = 3e-15


@pytest.mark.parametrize('n,decim', [(4096, 2), (4096, 4), (8192, 8)])
def test_folding_identity_full_support_table_rows(n, decim):
    rng = np.random.default_rng(7 * n + decim)
    x = rng.standard_normal(n)
    F = 4
    W = (rng.standard_normal((F, n)) + 1j * rng.standard_normal((F, n))) / np.sqrt(n)
    want = O.cwt_from_rows(x, list(W), False)[:, ::decim]
    got = folded_rows(W, x, decim)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f'table n={n} decim={decim}: {err:.2e}')
    assert err <= 1e-13
    # with the interpolate mask (X zeroed from N/2 up) folded into W, as the plan's table has it
    Wm = W.copy()
    Wm[:, n // 2:] = 0
    want_i = O.cwt_from_rows(x, list(W), True)[:, ::decim]
    got_i = folded_rows(Wm, x, decim)
    assert np.max(np.abs(got_i - want_i)) / np.max(np.abs(want_i)) <= 1e-13
