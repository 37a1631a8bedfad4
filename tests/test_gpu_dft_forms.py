"""GPU parity of every register-DFT instantiation the engines run (nw_dft_reg.h: radix-2 DIT
with FMA butterflies, the inter-pass twiddles folded into the first stage).

One-pass sizes: n = 1024 .. 16384, fp32 and fp64, cwt and power, S = 3 signals (the fp32
signal-pair kernel, its odd last signal and the single-signal kernels), Morse and Morlet, with
a frequency list picked so the rows run every pass-0 variant (pruned idft_br<T, E, NZ>) the
kernel instantiates.  Which variant a row runs follows from its support: the last bin above
kTailRel x the row's max |W| (nw_internal.h), rounded as wsupport_kernel / pass0_variant
(nw_fused.hip) round it.  nw_plan_row_support serves the two-pass engine's plans only (it fails
on a one-pass plan), so the supports here are read off the plan's own W rows with that rule
(tests/fused_variants.py, shared with the table rows' test); the set of variants hit must equal
the instantiated set -- a miss fails, it is not skipped.

Other forms: one chirp-z length (n = 1201) and the smallest two-pass length (n = 2^15, 4
scales; its rows' supports through nw_plan_row_support).

Tolerance: TOL of tests/test_gpu_parity.py, 1e-12 (fp64) / 1e-5 (fp32) of max |ref| against
oracle.nw_oracle, for cwt and power alike."""
import numpy as np
import pytest

from fused_variants import instantiated_variants, row_wnz, variant_of
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

TOL = {'float64': 1e-12, 'float32': 1e-5}
SFREQ = 1000.
S = 3
KINDS = {'morse': (nw.Morse, {}), 'morlet': (nw.Morlet, {})}
CANDIDATES = np.geomspace(0.6, 480.0, 160)


_picked = {}


def pick_freqs(kind, n, dtype):
    """One frequency per value of wnz that occurs for this (kind, n): the candidate whose
    support sits deepest inside its bucket, so fp32 / fp64 row rounding cannot move it."""
    key = (kind, n, dtype)
    if key not in _picked:
        cls, params = KINDS[kind]
        rows = cls(SFREQ, dtype='float64', **params).make_fft_wavelets(CANDIDATES, n / SFREQ)
        best = {}
        for f, row in zip(CANDIDATES, rows):
            wnz, need = row_wnz(row, n, dtype)
            margin = min(wnz - need, need - 1)          # distance to the bucket's ends
            if wnz not in best or margin > best[wnz][0]:
                best[wnz] = (margin, f)
        _picked[key] = {w: f for w, (_, f) in best.items()}
    return _picked[key]


def signals(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SFREQ
    fc = rng.uniform(2, 300, (S, 1))
    return np.sin(2 * np.pi * fc * t + rng.uniform(0, 6.28, (S, 1))) + 0.2 * rng.standard_normal((S, n))


_refs = {}


def reference(kind, n, freqs, x, dtype):
    key = (kind, n, tuple(freqs), dtype)
    if key not in _refs:
        _refs[key] = np.stack([O.cwt(kind, xi, np.asarray(freqs)) for xi in x])
    return _refs[key]


def check(got, ref, dtype, out, what):
    want = ref if out == 'cwt' else np.abs(ref) ** 2
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f'{what}: rel err {err:.3e} (tol {TOL[dtype]:.0e})')
    assert got.shape == want.shape
    assert err <= TOL[dtype], (what, err)


@pytest.mark.parametrize('out', ['cwt', 'power'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('kind', ['morse', 'morlet'])
@pytest.mark.parametrize('n', [1024, 2048, 4096, 8192, 16384])
def test_one_pass_every_pass0_variant(n, kind, dtype, out):
    by_wnz = pick_freqs(kind, n, dtype)
    freqs = sorted(by_wnz.values())
    # the kernels these calls run: fp32 at n <= 4096 pairs signals 0, 1 (pair kernel) and runs
    # the odd last one alone; everything else is the single-signal kernel
    kernels = [False, True] if (dtype == 'float32' and n <= 4096) else [False]
    for pair in kernels:
        variants = instantiated_variants(n, dtype, out, pair)
        hit = {variant_of(w, variants) for w in by_wnz}
        assert hit == variants, f'pass-0 variants hit {sorted(hit)} != instantiated {sorted(variants)} (pair={pair})'
    x = signals(n, 7 + n)
    cls, params = KINDS[kind]
    got = cls(SFREQ, dtype=dtype, **params).cwt_batch(x.astype(dtype), np.asarray(freqs), out=out)
    ref = reference(kind, n, freqs, x.astype(dtype).astype(np.float64), dtype)
    check(got, ref, dtype, out, f'{kind} n={n} {dtype} {out}')


@pytest.mark.parametrize('out', ['cwt', 'power'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_chirp_length(dtype, out):
    """n = 1201: the chirp-z kernel (two on-chip FFTs per row, pruned pass 0 NZ = 1, 2, 4, E/2)."""
    n = 1201
    freqs = [1.5, 7., 30., 120., 400.]
    x = signals(n, 3)
    got = nw.Morse(SFREQ, dtype=dtype).cwt_batch(x.astype(dtype), np.asarray(freqs), out=out)
    ref = reference('morse', n, freqs, x.astype(dtype).astype(np.float64), dtype)
    check(got, ref, dtype, out, f'chirp n={n} {dtype} {out}')


@pytest.mark.parametrize('out', ['cwt', 'power'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_smallest_two_pass_length(dtype, out):
    """n = 2^15, 4 scales: the row pass (pruned idft_br, twiddled passes) and the column pass."""
    n = 1 << 15
    freqs = np.array([3., 40., 150., 420.])
    p = nw.Plan(n, freqs.size, dtype)
    try:
        p.set_wavelet('morse', [17.5, 3.0], freqs, L.trans_grid(n / SFREQ, SFREQ, False))
        k = p.row_support()
    finally:
        p.close()
    assert np.all(np.diff(k) > 0) and k[0] > 0 and k[-1] < n, k     # four different supports, all cut
    x = signals(n, 11)
    got = nw.Morse(SFREQ, dtype=dtype).cwt_batch(x.astype(dtype), freqs, out=out)
    ref = reference('morse', n, list(freqs), x.astype(dtype).astype(np.float64), dtype)
    check(got, ref, dtype, out, f'two-pass n={n} {dtype} {out}')
