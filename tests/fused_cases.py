"""Inputs of the per-row tests of the one-pass kernels with real W rows (nw_fused_kernel<..., REALW =
true>, nw_fused_pair_kernel, fwd_r2c_kernel; nw_fused.hip): tests/test_gpu_fused_rows.py runs them
on the device, tests/test_fused_cases_cpu.py checks on the reference alone that they do what they
are meant to.  No test here.

Rows: analytic rows with a hard edge.  A plan's wavelet is set on the grid (delta = 1, len_full =
n, len_valid = K), so bin j holds psi(j) for j < K and exactly zero from K on (wavelet_bin,
nw_internal.h).  A plan has one K and F = 3 rows with peak frequencies 0.85 (K - 1), K - 1 and
1.3 (K - 1): the peak inside the support, on its edge, and a row still rising at the edge.  Kinds:
Morse (17.5, 3) and Morlet (sigma = 2, not Gabor), whose psi(0) is 0 (so K = 1 is left out).

Supports: with E = elems_per_thread(n) and TT = n / E, K = v TT and v TT + 1 for every v of
{1, 2, 4, 8, 12, 16, 20, 24, 28} below E, and K = n: both ends of every step of wnz_round
(nw_shape.h), so of every pass-0 variant and of every shifted value of the partial-sum kernels;
v = E / 2 puts the Nyquist bin just outside the row and just inside it.

Signals: S = 5 per case, flat magnitude spectrum (|X[k]| = sqrt(n) at every bin) with random
phases, rounded to the compute dtype; the reference sees the rounded values.  With white noise a
single bin can be small enough for its loss to hide under the bound.

Also restated here: which reductions form their sums as block partials inside the transform kernel
(kPSumOK / kPhSumOK, nw_shape.h) as a literal table, and group_filling (signals per block of the
single-signal output kernel) with its constants read from the header."""
import os
import re

import numpy as np

from fused_variants import elems_per_thread
from oracle import nw_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = {'float64': 1e-12, 'float32': 1e-5}      # the parity contract of tests/test_gpu_parity.py
SIZES = [1024, 2048, 4096, 8192, 16384]
DTYPES = ['float32', 'float64']
OUTS = ['cwt', 'abs', 'power']
S = 5
PEAKS = (0.85, 1.0, 1.3)
STEPS = (1, 2, 4, 8, 12, 16, 20, 24, 28)
# plan parameters of a kind, and the oracle's spectrum of it
KIND_PARAMS = {'morse': [17.5, 3.], 'morlet': [2., 0.]}
SPECTRUM = {'morse': lambda nu, f: O.morse_spectrum(nu, f, 17.5, 3.),
            'morlet': lambda nu, f: O.morlet_spectrum(nu, f, 2., False)}

# n at which power_sum / phase_sum are block partial sums of the transform kernel
# (NW_REDUCE_PARTIALS); per-signal rows added per chunk (NW_REDUCE_ROWS) elsewhere
PARTIALS = {('float32', 'power_sum'): {1024, 2048, 4096, 8192, 16384},
            ('float32', 'phase_sum'): {1024, 2048, 4096, 8192},
            ('float64', 'power_sum'): {1024, 2048, 4096, 8192},
            ('float64', 'phase_sum'): {1024, 2048, 4096, 8192}}


def pair_kernel(n, dtype):
    """Whether the signal-pair kernel writes the outputs of (n, dtype) (kPairMode, nw_shape.h)."""
    return dtype == 'float32' and n <= 4096


def tol_of(dtype, out):
    return TOL[dtype] * (2 if out == 'power' else 1)


def supports(n):
    """The K of the docstring, ascending: 11 at E = 16, 19 at E = 32."""
    e = elems_per_thread(n)
    tt = n // e
    return [k for v in STEPS if v < e for k in (v * tt, v * tt + 1)] + [n]


def pair_supports(n):
    """The K on either side of kPairWKeepRed = 10 and of the pass-0 variant 12 (nw_fused.hip)."""
    tt = n // elems_per_thread(n)
    return [8 * tt, 8 * tt + 1, 12 * tt, 12 * tt + 1]


def freqs_of(k):
    return np.array([p * (k - 1) for p in PEAKS])


def oracle_rows(kind, n, k):
    """(3, n) float64: the oracle's spectrum on the grid 0, 1, ..., cut after bin k - 1."""
    nu = np.arange(n, dtype=np.float64)
    rows = np.array([SPECTRUM[kind](nu, f) for f in freqs_of(k)])
    rows[:, k:] = 0.0
    return rows


_signals = {}


def signals(n, dtype, count=S, nyquist=None):
    """(count, n) in ``dtype``: irfft(exp(2 pi i u), n) sqrt(n) with the DC bin +1 and the Nyquist
    bin -1, u from default_rng(n).  ``nyquist``: a tuple of ``count`` signs for the Nyquist bins
    instead (the same signals otherwise)."""
    key = (n, dtype, count, nyquist)
    if key not in _signals:
        u = np.random.default_rng(n).random((count, n // 2 + 1))
        spec = np.exp(2j * np.pi * u)
        spec[:, 0], spec[:, -1] = 1.0, -1.0 if nyquist is None else np.asarray(nyquist, dtype=np.float64)
        x = (np.fft.irfft(spec, n, axis=-1) * np.sqrt(n)).astype(dtype)
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


# The Nyquist bin is -1 in every signal above (up to the rounding of the forward transform), and
# the kernels carry it one signal ahead in registers: a block that handed every signal the bin of
# its first signal would stay inside every bound.  Signs that differ inside every block of 2
# (S = 5) and inside every block of 8 (67 signals: -1 for the first signal of a block only):
NYQUIST_ALTERNATE = (-1., 1., -1., 1., -1.)


def nyquist_lead(count, group=8):
    return tuple(-1. if s % group == 0 else 1. for s in range(count))


def reference(x, rows):
    """(S, F, n) complex128 of the rows (F, n) as given."""
    return np.stack([O.cwt_from_rows(xi.astype(np.float64), list(np.asarray(rows, dtype=np.float64)), False)
                     for xi in x])


def as_kind(c, out):
    return c if out == 'cwt' else np.abs(c) if out == 'abs' else np.abs(c) ** 2


def row_max(ref):
    """(S, F): max |ref| of every (signal, row)."""
    return np.max(np.abs(ref), axis=-1)


def epoch_sums(ref):
    """power_sum (F, n) and phase_sum (F, n) complex of the reference, added in signal order."""
    ps = np.zeros(ref.shape[1:])
    ph = np.zeros(ref.shape[1:], dtype=np.complex128)
    for y in ref:
        ps += np.abs(y) ** 2
        ph += y / np.abs(y)
    return ps, ph


def power_sum_bound(ref, dtype):
    """(F, 1): a value of |y|^2 is off by at most 2 TOL max|row|^2 (part A), so their sum over the
    signals by at most 2 TOL sum_s max|ref_s row|^2."""
    return 2 * TOL[dtype] * np.sum(row_max(ref) ** 2, axis=0)[:, None]


def phase_sum_bound(ref, dtype):
    """(F, n): a phasor of a value known to TOL max|row| at magnitude |y| is off by at most
    2 TOL max|row| / |y| (to first order TOL max / |y|; the factor 2 covers the second order up to
    the cap PHASE_CAP), so the sum by at most 2 TOL sum_s max|ref_s row| / |ref_s[k]|."""
    with np.errstate(divide='ignore'):
        return 2 * TOL[dtype] * np.sum(row_max(ref)[:, :, None] / np.abs(ref), axis=0)


PHASE_CAP = 0.05       # phase points are checked where their bound is at most this ...
PHASE_SHARE = 0.9      # ... which at least this share of a case's points must be


def pair_sums(ya, yb):
    """(cross (F, n, 4) = {Re S_ab, Im S_ab, P_aa, P_bb}, phi (F, n)) of complex128 rows (E, F, n),
    added in pair order."""
    s = np.zeros(ya.shape[1:], dtype=np.complex128)
    paa, pbb = np.zeros(ya.shape[1:]), np.zeros(ya.shape[1:])
    phi = np.zeros(ya.shape[1:], dtype=np.complex128)
    for a, b in zip(ya, yb):
        s += a * np.conj(b)
        paa += np.abs(a) ** 2
        pbb += np.abs(b) ** 2
        phi += (a / np.abs(a)) * np.conj(b / np.abs(b))
    return np.stack([s.real, s.imag, paa, pbb], axis=-1), phi


# ---- signals per block of the single-signal output kernel -------------------------------------
def shape_constants():
    """kMinRounds, kResidentBlocks, kGroup and the fp64 block sizes as nw_shape.h defines them."""
    src = open(os.path.join(ROOT, 'ninwavelets_amd', 'csrc', 'nw_shape.h')).read()
    m = re.search(r'constexpr int64_t kMinRounds = (\d+), kResidentBlocks = (\d+);', src)
    return {'min_rounds': int(m.group(1)), 'resident': int(m.group(2)),
            'group': int(re.search(r'constexpr int kGroup = (\d+);', src).group(1)),
            'group64': int(re.search(r'#define NW_GROUP64 (\d+)', src).group(1)),
            'group64_16k': int(re.search(r'#define NW_GROUP64_16K (\d+)', src).group(1))}


def group_base(n, dtype, c=None):
    """kGroupOut (nw_shape.h): signals per block of a launch that fills the chip."""
    c = c or shape_constants()
    if dtype == 'float32':
        return c['group']
    return c['group64_16k'] if n == 16384 else c['group64']


def group_filling(base, nsig, nfreq, c=None):
    """group_filling (nw_shape.h): ``base`` halved (down to 2) while the launch would fill the
    chip fewer than kMinRounds times over."""
    c = c or shape_constants()
    g = base
    while g > 2 and -(-nsig // g) * nfreq < c['min_rounds'] * c['resident']:
        g //= 2
    return g
