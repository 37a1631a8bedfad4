"""GPU parity of the device-built WaveletMode.Normal tables (k_normal_time, one rocFFT per row length,
k_normal_finish: MexicanHat and Haar, base.py:249-256) against oracle.nw_oracle.fft_wavelets, past the one case of
test_gpu_parity.py (sfreq 1000, six scales): MexicanHat with sigma 7 and 3 and Haar, interpolate False and True, at
three (sfreq, real_length, real_wave_length) whose rows come in two lengths each (test_aux_cases_cpu.py asserts that
on the oracle), 999-point rows (27 x 37, no smooth rocFFT length) among them.

Rows: the lengths equal the oracle's, the values within 1e-13 max(1, row peak).  The CWT of two white-noise signals
through the tables against oracle.nw_oracle.cwt, every scale row against its own maximum at the parity tolerances
(1e-12 fp64, 1e-5 fp32): on the rocFFT engine at n = int(sfreq real_length), and on the one-pass kernel at n = 1024,
where every ragged row is centre-padded on its own."""
import numpy as np
import pytest

import aux_cases as A
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

from ninwavelets_amd import _lib as L  # noqa: E402

TOL = {'float64': 1e-12, 'float32': 1e-5}
CASE_IDS = [f'{s}-{rl}-{rwl}' for s, rl, rwl in A.NORMAL_CASES]


def wavelet(name, sfreq, rwl, interpolate, **kw):
    cls, ckw, _, _ = A.NORMAL_KINDS[name]
    return cls(sfreq, real_wave_length=rwl, interpolate=interpolate, **ckw, **kw)


@pytest.mark.parametrize('interpolate', [False, True])
@pytest.mark.parametrize('case', A.NORMAL_CASES, ids=CASE_IDS)
@pytest.mark.parametrize('name', list(A.NORMAL_KINDS))
def test_table_rows_against_the_oracle(name, case, interpolate):
    sfreq, real_length, rwl = case
    w = wavelet(name, sfreq, rwl, interpolate)
    assert w._device_normal() is not None
    got = w.make_fft_wavelets(A.NORMAL_FREQS, real_length)
    ref = A.normal_oracle_rows(name, sfreq, real_length, rwl, interpolate)
    assert [r.shape for r in got] == [r.shape for r in ref]
    assert len({len(r) for r in ref}) == 2
    worst = 0.0
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == r.dtype == np.complex128
        if interpolate:
            assert np.all(g[len(r) // 2:] == 0)
        err = np.max(np.abs(g - r)) / max(1.0, np.max(np.abs(r)))
        worst = max(worst, err)
        assert err <= 1e-13, (name, case, interpolate, A.NORMAL_FREQS[i], len(r), err)
    print(f'{name} {case} interpolate={interpolate}: lengths {[len(r) for r in ref]}, worst {worst:.2e}')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('interpolate', [False, True])
@pytest.mark.parametrize('case', A.NORMAL_CASES, ids=CASE_IDS)
@pytest.mark.parametrize('name', list(A.NORMAL_KINDS))
def test_cwt_through_the_tables(name, case, interpolate, dtype):
    sfreq, real_length, rwl = case
    _, _, kind, okw = A.NORMAL_KINDS[name]
    for n, engine, kernel in ((int(sfreq * real_length), 'rocfft', 'k1_multiply'), (1024, None, 'nw_fused_kernel')):
        x = np.random.default_rng(6200 + n).standard_normal((2, n)).astype(dtype)
        w = wavelet(name, sfreq, rwl, interpolate, dtype=dtype, engine=engine)
        for s in x:
            got = w.cwt(s, A.NORMAL_FREQS)
            ref = O.cwt(kind, s.astype(np.float64), A.NORMAL_FREQS, sfreq, interpolate, rwl, **okw)
            assert got.shape == ref.shape
            err = np.max(np.abs(got - ref), axis=-1) / np.max(np.abs(ref), axis=-1)        # per scale row
            print(f'{name} {case} interpolate={interpolate} {dtype} n={n}: worst row {err.max():.2e} '
                  f'({A.NORMAL_FREQS[int(err.argmax())]} Hz)')
            assert err.max() <= TOL[dtype], (name, case, interpolate, dtype, n, err)
        ran = {L.KERNEL_NAMES[p.stats()['kernel']] for p in w._plans.values()}
        assert ran == {kernel}, ran
