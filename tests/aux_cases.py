"""What the tests of the older kernels share: the wavelet row evaluators psi_f32 / psi_f64 / k_rows
(test_gpu_wavelet_rows.py), the time-domain wavelets of nw_make_wavelets (test_gpu_make_wavelets.py), the
device-built Normal tables (test_gpu_normal_tables.py) and nw_baseline (test_gpu_baseline.py), with the CPU checks of
the cases themselves (test_aux_cases_cpu.py).

Here, once each: the scale list and the parameter sets of the row tests, the numpy float32 restatement of psi_f32
and the floor it gives the fp32 row bound (floor_of: CPU arithmetic only, never a device result), the sweep of the
time-domain wavelets, the Normal-table cases, and the record the tests keep of what they measure (record)."""
import os

import numpy as np

from oracle import nw_oracle as O

import ninwavelets_amd as nw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'profiles', 'r21_aux_cases.txt')

FREQS40 = np.geomspace(0.6, 480., 40)
MORSE_SETS = [(17.5, 3), (3, 2), (10, 2), (0.5, 1), (1, 3), (40, 3), (60, 3), (17.5, 1), (17.5, 8), (5, 0.5)]
MORLET_SETS = [(7, False), (7, True), (5, False), (2, False), (12, False), (20, False)]
ROW_SETS = [('morse', p) for p in MORSE_SETS] + [('morlet', p) for p in MORLET_SETS]
ROW_N = 4096                       # the row tests' plan length (sfreq 1000)


def set_id(case):
    kind, p = case
    return f'morse-b{p[0]:g}-r{p[1]:g}' if kind == 'morse' else f'morlet-s{p[0]:g}' + ('-gabor' if p[1] else '')


def plan_params(kind, params):
    """The parameter list nw_plan_set_wavelet takes for a set: Morse [b, r]; Morlet [sigma, gabor, c, k] as the
    class holds them (wavelets.py:118-122)."""
    if kind == 'morse':
        return [float(params[0]), float(params[1])]
    if kind == 'morlet':
        c, k = O.morlet_constants(float(params[0]), bool(params[1]))
        return [float(params[0]), 1.0 if params[1] else 0.0, float(c), float(k)]
    return []


def oracle_params(kind, params):
    if kind == 'morse':
        return dict(b=float(params[0]), r=float(params[1]))
    if kind == 'morlet':
        return dict(sigma=float(params[0]), gabor=bool(params[1]))
    return {}


f32 = np.float32


def _fma32(a, b, c):
    """fma(a, b, c) of float32 values: the product of two float32 is exact in float64, the sum rounds to 53 bits
    and then to 24 (the second rounding moves a result only when the first landed on a float32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def psi32_restated(kind, params, j, delta, freq):
    """psi_f32 (nw_internal.h) in numpy float32, operation for operation; j: integer bins, delta: the grid
    spacing, freq: the scale.  numpy's log2 / exp2 / exp stand for the device's."""
    j = np.asarray(j).astype(f32)
    with np.errstate(all='ignore'):
        if kind == 'morse':
            b, r = float(params[0]), float(params[1])
            c1 = f32((b / r) * 1.4426950408889634)
            x = j * f32(delta / freq)
            lx = np.log2(x)
            lq = c1 * (f32(1) - np.exp2(f32(r) * lx))
            e2 = _fma32(np.full_like(lx, f32(b)), lx, lq)
            return np.where(x > 0, f32(2) * np.exp2(e2), f32(0)).astype(f32)
        sigma, gabor = float(params[0]), bool(params[1])
        c, k = O.morlet_constants(sigma, gabor)
        cpi, kappa = f32(c * np.float_power(np.pi, -1 / 4)), f32(k)
        x = j * f32(delta / freq * O.morlet_peak(sigma, freq))
        a = f32(sigma) - x
        return (cpi * (np.exp(-(a * a) * f32(0.5)) - kappa * np.exp(-(x * x) * f32(0.5)))).astype(f32)


_FLOORS = {}


def floor_rows(kind, params, n=ROW_N, sfreq=1000., freqs=FREQS40):
    """Per scale, max_j |psi32_restated - oracle| / the oracle row's peak on trans_grid(sfreq, n / sfreq, False);
    NaN for a scale whose oracle row holds a non-finite bin (Morse b = 100: x^b overflows fp64)."""
    nu = O.trans_grid(sfreq, n / sfreq, False)
    delta = 1 / (n / sfreq)
    out = []
    for f in freqs:
        with np.errstate(all='ignore'):
            ref = (O.morse_spectrum(nu, f, *map(float, params)) if kind == 'morse'
                   else O.morlet_spectrum(nu, f, float(params[0]), bool(params[1])))
            got = psi32_restated(kind, params, np.arange(len(nu)), delta, f)
            out.append(np.max(np.abs(got.astype(np.float64) - ref)) / np.max(np.abs(ref))
                       if np.all(np.isfinite(ref)) else np.nan)
    return np.array(out)


def floor_of(kind, params):
    """The fp32 floor of a parameter set: the largest of floor_rows over the scales of FREQS40 whose oracle row is
    finite (every scale, for the sets of ROW_SETS), at n = 4096, sfreq 1000."""
    key = (kind, tuple(params))
    if key not in _FLOORS:
        _FLOORS[key] = float(np.nanmax(floor_rows(kind, params)))
    return _FLOORS[key]


OVERFLOW_SET = ('morse', (100, 3))        # x^b overflows fp64 at the low scales: inf and NaN bins
OVERFLOW_FREQS = [0.5, 0.8, 3., 60.]


# ---------------------------------------------------------------------------------------------------------
# time-domain wavelets: (sfreq, real_wave_length) x kinds on nine scales
# ---------------------------------------------------------------------------------------------------------
SWEEP = [(1000, 1), (999, 1), (1001, 1), (333, 1.5), (250, 1), (1000, 0.301)]
SWEEP_FREQS = [0.7, 1, 3.3, 7, 13.7, 40, 97.3, 211, 433]
# name -> (class, its keywords, the oracle's kind, the oracle's keywords)
SWEEP_KINDS = {'morse': (nw.Morse, {}, 'morse', {}),
               'morse_b3_r2': (nw.Morse, dict(b=3., r=2.), 'morse', dict(b=3., r=2.)),
               'shannon': (nw.Shannon, {}, 'shannon', {}),
               'morlet': (nw.Morlet, {}, 'morlet', {}),
               'morlet_s5': (nw.Morlet, dict(sigma=5.), 'morlet', dict(sigma=5.)),
               'morlet_gabor': (nw.Morlet, dict(gabor=True), 'morlet', dict(gabor=True)),
               'mexican_hat': (nw.MexicanHat, {}, 'mexican_hat', {}),
               'haar': (nw.Haar, {}, 'haar', {})}


def sweep_wavelet(name, sfreq, rwl):
    cls, kw, _, _ = SWEEP_KINDS[name]
    return cls(sfreq, real_wave_length=rwl, **kw)


def sweep_oracle(name, freqs, sfreq, rwl):
    _, _, kind, okw = SWEEP_KINDS[name]
    return O.make_wavelets(kind, freqs, sfreq=sfreq, real_wave_length=rwl, **okw)


def reverse_m(freq, sfreq, rwl):
    """The spectrum length m of a Reverse-kind wavelet before the conj-flip slice (base.py:191-194)."""
    return len(np.arange(0, sfreq / freq * rwl, 1 / freq))


# ---------------------------------------------------------------------------------------------------------
# device-built Normal tables: (sfreq, real_length, real_wave_length) x kinds on the sweep's scales
# ---------------------------------------------------------------------------------------------------------
NORMAL_CASES = [(999, 1.3, 1), (250, 4.1, 2), (1000, 2.048, 1)]
NORMAL_KINDS = {'mexican_hat_s7': (nw.MexicanHat, dict(sigma=7.), 'mexican_hat', dict(sigma=7.)),
                'mexican_hat_s3': (nw.MexicanHat, dict(sigma=3.), 'mexican_hat', dict(sigma=3.)),
                'haar': (nw.Haar, {}, 'haar', {})}
# (5.7 and 42.6 Hz: scales at which Haar's timeline, otherwise sfreq samples, has one more)
NORMAL_FREQS = [0.7, 3.3, 5.7, 13.7, 42.6, 97.3, 211]


def normal_oracle_rows(name, sfreq, real_length, rwl, interpolate):
    _, _, kind, okw = NORMAL_KINDS[name]
    return O.fft_wavelets(kind, NORMAL_FREQS, sfreq, real_length, interpolate, rwl, **okw)


# ---------------------------------------------------------------------------------------------------------
# the record
# ---------------------------------------------------------------------------------------------------------
_HEAD = ('# Tests of the wavelet row evaluators, nw_make_wavelets, the device-built Normal tables and nw_baseline\n'
         '# (tests/aux_cases.py): what the tests measure.  Each section is rewritten by the test named in its\n'
         '# heading whenever that test runs; sections of GPU tests hold figures of a gfx950 (MI355X) run.\n')


def record(section, lines):
    """Replace (or add) the section ``section`` of the record with ``lines``.  A tree that cannot be written to
    keeps its record as it is: what the tests assert does not depend on the file."""
    try:
        text = open(RECORD).read() if os.path.exists(RECORD) else _HEAD
        parts = text.split('\n## ')
        head, secs = parts[0], {}
        for p in parts[1:]:
            title, _, body = p.partition('\n')
            secs[title] = body.rstrip('\n')
        secs[section] = '\n'.join(lines)
        with open(RECORD, 'w') as fh:
            fh.write(head.rstrip('\n') + '\n')
            for title in sorted(secs):
                fh.write(f'\n## {title}\n{secs[title]}\n')
    except OSError:
        pass
