"""What the tests of the epoch-chunk reductions share: signal pairs (test_gpu_pair.py / test_pair_cpu.py),
connectivity (test_gpu_conn.py / test_conn_cpu.py), phase lag (test_gpu_lag.py / test_lag_cpu.py), over-time
connectivity (test_gpu_conn_time.py / test_conn_time_cpu.py), envelope correlation (test_gpu_env.py /
test_env_cpu.py) and phase-amplitude coupling (test_gpu_pac.py / test_pac_cpu.py).

Here, once each: the scale lists and the tolerances every documented bound rests on (tol_of, vis_of), the input
recipes with their oracle rows (oracle_rows, pair_rows), the Morse plan, the engine-form table (FORMS, forms), the
over-time windows and the kernels' summation order (windows_of, lane_sum), the epochs stand-in (FakeEpochs, also
test_gpu_decim.py's and test_gpu_parity.py's) and the child process of the debug-library tests
(run_under_bounds_checks).  The reference arithmetic of each reduction (sums_of, lag_of, ref_sums, own_sums,
ref_env, check_t1, ...) is what its file tests and stays there."""
import os
import subprocess
import sys
from functools import partial

import numpy as np

from oracle import nw_oracle as O

import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import time_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, 'ninwavelets_amd', 'libninwave_debug.so')

FREQS = [4., 7., 12., 20., 40., 70., 120., 200., 300.]     # nine scales: one more than a tile
FREQS3 = [3., 30., 200.]
CHIRP = (1201,)                     # lengths the tests run on the chirp-z form


def tol_of(n, dtype):
    """The per-signal contract: max |y - ref| <= tol max |ref| over a signal's (F, N) rows."""
    if dtype == 'float64':
        return 1e-12
    return 2e-5 if n in CHIRP else 1e-5


def vis_of(dtype):
    """The share of A_a A_b below which the sign of Im y_a conj(y_b) may flip (2.5 x the largest perturbation
    2 tol at the chirp tolerance in fp32)."""
    return 1e-9 if dtype == 'float64' else 1e-4


_ROWS = {}


def _cwt_rows(x, rows):
    return np.stack([O.cwt_from_rows(s.astype(np.float64), rows, False) for s in x])


def _shared(key, make):
    """make()'s arrays, computed once per key and shared read-only."""
    if key not in _ROWS:
        arrays = make()
        for a in arrays:
            a.setflags(write=False)
        _ROWS[key] = arrays
    return _ROWS[key]


SEEDS = {'plain': 2300, 'lagged': 2300, 'coupled': 2600}


def oracle_rows(recipe, n, E, C, dtype, freqs):
    """(x, y): the inputs (E, C, n) in the compute dtype and their complex128 CWT rows (E, C, F, n), computed
    once per case and shared (read-only).  rng = default_rng(SEEDS[recipe] + n), common = standard_normal
    (E, 1, n), then noise = standard_normal (E, C, n):
      'plain'    x = 0.6 common + 0.8 noise
      'lagged'   x[:, c] = 0.6 roll(common, 3 c) + 0.8 noise[:, c], so that the sign sums are not centred on 0
      'coupled'  the lagged one, then phases = uniform(0, 2 pi, E) and every even channel also gets
                 2 cos(phi) + 1.5 (1 + 0.9 cos(phi)) cos(2 pi 70 t + 1), phi = 2 pi 7 t + the epoch's phase: a
                 70 Hz amplitude that follows the 7 Hz phase (sfreq 1000)"""
    def make():
        rng = np.random.default_rng(SEEDS[recipe] + n)
        common = rng.standard_normal((E, 1, n))
        noise = rng.standard_normal((E, C, n))
        if recipe == 'plain':
            x = 0.6 * common + 0.8 * noise
        else:
            x = np.stack([0.6 * np.roll(common[:, 0], 3 * c, axis=-1) + 0.8 * noise[:, c] for c in range(C)], axis=1)
        if recipe == 'coupled':
            t = np.arange(n) / 1000.
            phi = 2 * np.pi * 7 * t + rng.uniform(0., 2 * np.pi, E)[:, None]                  # (E, n)
            x[:, 0::2] += (2 * np.cos(phi) + 1.5 * (1 + 0.9 * np.cos(phi)) * np.cos(2 * np.pi * 70 * t + 1))[:, None]
        x = x.astype(dtype)
        rows = O.fft_wavelets('morse', freqs, 1000., n / 1000., False)
        return x, np.stack([_cwt_rows(ep, rows) for ep in x])
    return _shared((recipe, n, E, C, dtype, tuple(freqs)), make)


plain_rows = partial(oracle_rows, 'plain')
lagged_rows = partial(oracle_rows, 'lagged')
coupled_rows = partial(oracle_rows, 'coupled')


def pair_rows(n, E, dtype, freqs, zero_b=None):
    """(a, b, ya, yb): two signals (E, n) in the compute dtype and their complex128 CWT rows (E, F, n), computed
    once per case and shared (read-only).  rng = default_rng(2100 + n), a = standard_normal (E, n),
    b = 0.6 a + 0.8 standard_normal (E, n); epoch ``zero_b`` of b all zero."""
    def make():
        rng = np.random.default_rng(2100 + n)
        a = rng.standard_normal((E, n))
        b = 0.6 * a + 0.8 * rng.standard_normal((E, n))
        a, b = a.astype(dtype), b.astype(dtype)
        if zero_b is not None:
            b[zero_b] = 0
        rows = O.fft_wavelets('morse', freqs, 1000., n / 1000., False)
        return a, b, _cwt_rows(a, rows), _cwt_rows(b, rows)
    return _shared(('pair', n, E, dtype, tuple(freqs), zero_b), make)


def morse_plan(n, dtype, freqs, max_batch, **kw):
    """A plan of Morse(1000)'s default b, r on the scales ``freqs`` (sfreq 1000)."""
    p = nw.Plan(n, len(freqs), dtype, max_batch=max_batch, **kw)
    p.set_wavelet('morse', [17.5, 3.], np.asarray(freqs), L.trans_grid(n / 1000., 1000., False))
    return p


# The engine forms a reduction is run on: (id, n, dtype, plan keywords, device decim, host step, kernel of the form
# as stats() names it).  A test file picks its rows by id (forms) and adds its own columns: epochs, channels, scales.
FORMS = [('1024-f32', 1024, 'float32', {}, 1, 1, 'nw_fused_pair_kernel'),
         ('1024-f64', 1024, 'float64', {}, 1, 1, 'nw_fused_kernel'),
         ('chirp-1201-f32', 1201, 'float32', {}, 1, 1, 'nw_chirp_kernel'),         # tail tile: 49 samples
         ('chirp-1201-f64', 1201, 'float64', {}, 1, 1, 'nw_chirp_kernel'),
         ('decim-4096', 4096, 'float32', {}, 4, 1, 'nw_fused_decim_kernel'),
         ('e32-8192', 8192, 'float32', {}, 1, 1, 'nw_fused_kernel'),
         ('rocfft-1000', 1000, 'float32', {'engine': 'rocfft'}, 1, 1, 'k1_multiply'),
         # the over-time calls on a full-rate plan summing every fourth sample
         ('rocfft-1000-step4', 1000, 'float32', {'engine': 'rocfft'}, 1, 4, 'k1_multiply'),
         ('twopass-32768', 32768, 'float32', {}, 1, 1, 'cols_kernel'),              # 512 sample tiles
         # more than 16 channels: three pair tiles, some of them partial
         ('tiles-17ch-f64', 1024, 'float64', {}, 1, 1, 'nw_fused_kernel')]


def forms(*ids):
    """The rows of FORMS with these ids, in this order."""
    by_id = {f[0]: f for f in FORMS}
    return [by_id[i] for i in ids]


# The rows of the reductions along the epoch axis (connectivity, phase lag) and of those over time within an epoch
# (over-time connectivity, envelope correlation; phase-amplitude coupling with a tile row of its own), and
# (E, C, freqs) of the rows that do not take a file's own number of epochs, five channels and the nine scales
EPOCH_AXIS = ('1024-f32', '1024-f64', 'chirp-1201-f32', 'chirp-1201-f64', 'decim-4096', 'e32-8192', 'rocfft-1000',
              'twopass-32768', 'tiles-17ch-f64')
OVER_TIME = ('1024-f32', '1024-f64', 'chirp-1201-f32', 'chirp-1201-f64', 'decim-4096', 'rocfft-1000-step4',
             'twopass-32768', 'tiles-17ch-f64')
SHAPES = {'twopass-32768': (2, 3, FREQS3), 'tiles-17ch-f64': (3, 17, FREQS3)}


def windows_of(n, n_out, host_decim):
    """(name, (t0, t1), step) in the plan's output samples."""
    if host_decim > 1:                       # a full-rate plan summing every host_decim-th sample
        out = []
        for name, w in (('full', None), ('one', (0, 1)), ('inner', (37, min(1001, n))), ('empty', (500, 500))):
            t0, t1, step, _ = time_window(n, host_decim, w, False)
            out.append((name, (t0, t1), step))
        return out
    # (stride: not one of the listed windows; the step > 1 addressing on every form, bit for bit in T2)
    return [('full', (0, n_out), 1), ('one', (0, 1), 1), ('inner', (37, 1001), 1), ('empty', (500, 500), 1),
            ('stride', (5, n_out - 3), 4)]


def lane_sum(terms):
    """The contract's sum of ``terms`` (..., T) along the last axis: 64 lane sums, lane l adding j = l,
    l + 64, ... in order from +0.0, then v = v[:h] + v[h:] for h = 32 .. 1.  (A lane or tail sample
    without a j < T adds nothing: padding with +0.0 is the same, an accumulator never being -0.0.)"""
    T = terms.shape[-1]
    ntl = -(-T // 64)
    pad = np.zeros(terms.shape[:-1] + (ntl * 64,))
    pad[..., :T] = terms
    pad = pad.reshape(terms.shape[:-1] + (ntl, 64))
    v = np.zeros(terms.shape[:-1] + (64,))
    for it in range(ntl):
        v = v + pad[..., it, :]
    h = 32
    while h >= 1:
        v = v[..., :h] + v[..., h:]
        h //= 2
    return v[..., 0]


class FakeEpochs:
    """What EpochsWavelet reads of an mne Epochs object."""

    def __init__(self, data, sfreq, ch_names):
        self._d, self.info, self.ch_names = data, {'sfreq': sfreq}, list(ch_names)

    def get_data(self):
        return self._d


_PREAMBLE = ('import sys; sys.path.insert(0, %r)\n'
             'import numpy as np\n'
             'import ninwavelets_amd as nw\n'
             'from ninwavelets_amd import _lib as L\n'
             'print("debug", L.lib().nw_debug_bounds())\n') % ROOT


def run_under_bounds_checks(body):
    """The stdout lines of a child python that runs ``body`` (after _PREAMBLE's imports) on the debug library
    (kernel bounds checks, nw_dcheck.h; NINWAVE_LIB picks the library at load time): it ended with status 0, so
    no check failed, and the library it loaded is the debug one."""
    env = dict(os.environ, NINWAVE_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, '-u', '-c', _PREAMBLE + body], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert 'debug 1' in lines, r.stdout
    return lines
