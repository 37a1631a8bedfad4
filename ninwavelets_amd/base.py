"""Drop-in ``WaveletBase`` / ``WaveletMode`` running the CWT on MI355X.

Mirrors the reference's L2 engine (base.py:126-443): same constructor
arguments, the same stateful, *unkeyed* wavelet cache (``reuse=True`` keeps the
first table whatever ``freqs`` or length later calls pass, base.py:394-397),
the same exceptions, the same pad/crop of the cached rows to the current
signal length and the same output dtypes (complex128 / float64 by default).

What changes is where the work runs.  The cache is a *descriptor*: for the
analytic wavelets (Morse, Morlet, Shannon) it is (kind, params, freqs, grid)
and the spectrum is evaluated inside the HIP kernels; for time-domain
(WaveletMode.Normal) wavelets and user plugins that override
``trans_formula``/``formula``, the host evaluates the rows once with the
plugin's own Python formula (the reference's plugin protocol, README.md:342-355)
and they are uploaded as a table.  fft -> multiply -> inverse fft -> |.|^2 run
in libninwave.so; there is no CPU compute path.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from enum import Enum
from functools import partial

import numpy as np
from scipy.fftpack import fft, ifft

from . import _lib as L
from .engine import (CONN_OUTS, ENV_OUTS, ERPAC_OUTS, LAG_OUTS, PAC_BIN_OUTS, PAC_OUTS, PAC_SURR_STATS, PAIR_OUTS, REDUCTIONS,
                     Plan, check_decim, check_indices, check_lags, check_nbins, check_pac_indices, check_scales, draw_lags,
                     execute_multi, finalize_conn, finalize_conn_time, finalize_env, finalize_erpac, finalize_lag, finalize_pac,
                     finalize_pac_bins, finalize_pac_surr, finalize_pair, np_dtype, time_window)
from .engine import make_wavelets as _make_wavelets_dev

# Device working-set budget per plan chunk (bytes); signals are streamed through it.
CHUNK_BYTES = int(os.environ.get('NINWAVE_CHUNK_BYTES', str(4 << 30)))
# Device bytes the plans cached by one wavelet object may hold together (nw_stats.device_bytes).
# Plans are keyed on (n, batch, device, ...): a session whose epoch lengths or batch sizes vary
# creates a plan per combination, so the least recently used ones are destroyed (their buffers
# freed) once the total exceeds this; the plans of the current call are always kept.
PLAN_CACHE_BYTES = int(os.environ.get('NINWAVE_PLAN_CACHE_BYTES', str(16 << 30)))


class WaveletMode(Enum):
    """Which spectrum source a wavelet uses (base.py:126-142)."""
    Normal = 0            # time-domain formula -> FFT table
    Both = 1              # analytic spectrum (time formula also available)
    Reverse = 2           # analytic spectrum only
    Indifferentiable = 3
    Twice = 4


def pad_to(wave_from: np.ndarray, wave_to: np.ndarray) -> np.ndarray:
    """Crop or centre-pad ``wave_from`` to ``wave_to.shape[0]`` (base.py:75-82)."""
    m, n = wave_from.shape[0], wave_to.shape[0]
    if m > n:
        return wave_from[:n]
    lo = (n - m) // 2
    return np.pad(wave_from, [lo, n - m - lo], 'constant')


def interpolate_alias(wave: np.ndarray, cuda: bool = False) -> np.ndarray:
    """Zero everything from bin int(len/2) up (base.py:107-123)."""
    keep = int(wave.shape[0] / 2)
    return np.pad(wave[:keep], [0, wave.shape[0] - keep], 'constant')


class _Cache:
    """The wavelet cache of one make_fft_wavelets call (base.py:258-279)."""

    _version = 0

    def __init__(self, kind, params, freqs, grid, table=None, row_len=None):
        _Cache._version += 1
        self.version = _Cache._version
        self.kind, self.params, self.freqs, self.grid, self.table = kind, params, freqs, grid, table
        if row_len is None and table is not None:
            row_len = np.full(table.shape[0], table.shape[1], dtype=np.int64)
        self.row_len = row_len


def _epochs(waves):
    """``waves`` as an (E, C, N) array, with E, C and N."""
    waves = np.asarray(waves)
    if waves.ndim != 3:
        raise ValueError(f'waves must be (epochs, channels, N); got shape {waves.shape}')
    return (waves, *waves.shape)


class WaveletBase:
    """Base class of the wavelets (base.py:145-443).

    Extra keyword arguments (not in the reference):
      dtype   -- compute dtype, 'float64' (default: the reference's arithmetic) or
                 'float32' (2x less HBM traffic; results within 1e-5 of max|ref|)
      device  -- HIP device index for single-device calls
      devices -- list of devices: batched calls shard signals over them
      engine  -- 'auto' (fused where supported), 'fused' or 'rocfft'
    ``cuda`` is accepted for compatibility; the GPU is always used.
    """

    def __init__(self, sfreq: float = 1000, real_wave_length: float = 1.,
                 interpolate: bool = True, cuda: bool = False, *, dtype='float64',
                 device: int = 0, devices=None, engine: str | None = None) -> None:
        self.mode: WaveletMode = WaveletMode.Normal
        self.sfreq: float = sfreq
        self.help: str = ''
        self.real_wave_length: float = real_wave_length
        self.interpolate = interpolate
        self.cuda = cuda
        self.dtype = np_dtype(dtype)
        self.device = device
        self.devices = list(devices) if devices else None
        self.engine = engine
        self._cache: _Cache | None = None
        self._rows = None
        self._plans: OrderedDict = OrderedDict()     # least recently used first
        self.plan_cache_bytes = PLAN_CACHE_BYTES

    # ------------------------------------------------------------------ plugin API
    def peak_freq(self, freq: float) -> float:
        return 1.

    def formula(self, timeline: np.ndarray, freq: float) -> np.ndarray:
        """Time-domain wavelet (override in plugins; base.py:281-302)."""
        return timeline

    def trans_formula(self, freqs: np.ndarray, freq: float = 1.) -> np.ndarray:
        """Frequency-domain wavelet (override in plugins; base.py:304-323)."""
        return freqs

    def cp_trans_formula(self, freqs: np.ndarray, freq: float = 1.) -> np.ndarray:
        """The reference's cupy twin (base.py:325-344); host arrays here."""
        return self.trans_formula(freqs, freq)

    def _analytic(self):
        """(kind, params) when the stock analytic spectrum applies, else None."""
        return None

    def _device_normal(self):
        """(kind, params) when the stock time-domain formula applies (the table is then
        built on the device), else None (plugin formulas: host-built table)."""
        return None

    # ------------------------------------------------------------------ grids
    def _setup_trans_shape(self, freq: float, real_wave_length: float,
                           cuda: bool = False) -> np.ndarray:
        """Frequency grid (base.py:173-194)."""
        return np.arange(0, self.sfreq / freq * real_wave_length, 1 / freq)

    def _setup_waveletshape(self, freq: float, real_length: float = 1,
                            zero_mean: bool = False) -> np.ndarray:
        """Time grid of the time-domain wavelet (base.py:196-216)."""
        p = self.peak_freq(freq)
        span = real_length / p * freq * 2 * np.pi
        step = 1 / self.sfreq * 2 * np.pi * freq / p
        return np.arange(-span / 2, span / 2, step) if zero_mean else np.arange(0, span, step)

    # ------------------------------------------------------------------ wavelets
    def _time_formula_spec(self):
        """(kind, params) when the stock time-domain formula applies (override)."""
        return None

    def _device_wavelet_spec(self):
        """(kind, params) of nw_make_wavelets for this wavelet, None for plugin formulas."""
        if self.mode in (WaveletMode.Reverse, WaveletMode.Twice):
            a = self._analytic()
            return a if a is not None and a[0] in ('morse', 'shannon') else None
        return self._time_formula_spec()

    def _device_wavelets(self, spec, freqs) -> list:
        kind, params = spec
        rows = _make_wavelets_dev(kind, params, freqs, self.sfreq, self.real_wave_length, self.device)
        return [r.real.copy() for r in rows] if kind in ('mexican_hat', 'haar') else rows

    def make_wavelet(self, freq: float) -> np.ndarray:
        """Time-domain wavelet (base.py:346-359): on the device for the stock wavelets."""
        if freq == 0:
            raise ZeroDivisionError
        spec = self._device_wavelet_spec()
        if spec is not None:
            return self._device_wavelets(spec, [freq])[0]
        if self.mode in (WaveletMode.Reverse, WaveletMode.Twice):
            w = ifft(self.trans_formula(self._setup_trans_shape(freq, self.real_wave_length)))
            half = int(w.shape[0])
            both = np.hstack((np.conj(np.flip(w)), w))
            return both[half // 2: half // 2 * 3]
        return self.formula(self._setup_waveletshape(freq, 1, zero_mean=True), freq)

    def make_wavelets(self, freqs) -> list:
        """List of time-domain wavelets (base.py:361-376): one device call for the stock
        wavelets (nw_make_wavelets), the plugin's own formula otherwise."""
        spec = self._device_wavelet_spec()
        if spec is not None:
            fr = list(freqs)
            if any(f == 0 for f in fr):
                raise ZeroDivisionError
            self.wavelets = self._device_wavelets(spec, fr)
        else:
            self.wavelets = [self.make_wavelet(f) for f in freqs]
        return self.wavelets

    def _normal_row(self, freq: float) -> np.ndarray:
        """Spectrum of the zero-padded time-domain wavelet, |Re|+i|Im| (base.py:249-256)."""
        w = self.make_wavelet(freq)
        half = int((self.sfreq * self.real_wave_length - w.shape[0]) / 2)
        spec = fft(np.hstack((np.zeros(half), w, np.zeros(half))))
        return np.abs(spec.real) + 1j * np.abs(spec.imag)

    def make_fft_wavelet(self, freq: float, real_length: float = 1.) -> np.ndarray:
        """One cached row, host-evaluated (base.py:221-256).  cwt() does not use
        this: it evaluates the analytic rows on the device."""
        if freq == 0:
            raise ZeroDivisionError
        if self.mode in (WaveletMode.Reverse, WaveletMode.Both):
            rl = real_length / 2 if self.interpolate else real_length
            t = self._setup_trans_shape(real_length, rl)
            row = self.trans_formula(t, freq)
            return np.hstack((row, np.zeros(len(t)))) if self.interpolate else row
        return self._normal_row(freq)

    def _build_cache(self, freqs, real_length: float) -> _Cache:
        self.freq_dist = freqs[1] - freqs[0]          # IndexError / TypeError as base.py:272
        fr = np.asarray(list(freqs), dtype=np.float64)
        spectral = self.mode in (WaveletMode.Reverse, WaveletMode.Both)
        analytic = self._analytic() if spectral else None
        if analytic is not None:
            if np.any(fr == 0):
                raise ZeroDivisionError
            kind, params = analytic
            cache = _Cache(kind, params, fr, L.trans_grid(real_length, self.sfreq, self.interpolate))
        elif not spectral and self._device_normal() is not None:
            if np.any(fr == 0):
                raise ZeroDivisionError                  # make_wavelet, base.py:234-235
            kind, params = self._device_normal()
            cache = _Cache(kind, params, fr, L.nw_grid(1.0, 0, 0))
        else:
            rows = [self.make_fft_wavelet(f, real_length) for f in fr]
            if self.interpolate:
                rows = [interpolate_alias(r) for r in rows]
            cache = self._table_cache(rows, fr)
        self._cache = cache
        self._rows = None
        return cache

    @staticmethod
    def _table_cache(rows, freqs) -> _Cache:
        rows = [np.asarray(r) for r in rows]
        lens = np.array([r.shape[0] for r in rows], dtype=np.int64)
        m = int(lens.max()) if len(rows) else 0
        table = np.zeros((len(rows), m), dtype=np.complex128)   # rows left-aligned
        for i, r in enumerate(rows):
            table[i, :r.shape[0]] = r
        grid = L.nw_grid(1.0, m, m)
        return _Cache('table', [], freqs, grid, table, lens)

    def make_fft_wavelets(self, freqs, real_wave_length: float = 1.) -> list:
        """Build (and return) the cached rows (base.py:258-279)."""
        self._build_cache(freqs, real_wave_length)
        return self.fft_wavelets

    @property
    def fft_wavelets(self) -> list:
        """The cached rows as the reference stores them (evaluated on the device
        for the analytic kinds)."""
        c = self._cache
        if c is None:
            raise AttributeError('fft_wavelets')
        if self._rows is None:
            if c.kind == 'table':
                self._rows = [row[:n] for row, n in zip(c.table, c.row_len)]
            else:
                plan = Plan(max(1, c.grid.len_full), len(c.freqs), 'float64', self.device,
                            interpolate=self.interpolate)   # Normal tables apply the alias mask
                plan.set_wavelet(c.kind, c.params, c.freqs, c.grid)
                rows = plan.rows()
                lens = getattr(plan, 'row_len', None)
                plan.close()
                self._rows = ([row[:n] for row, n in zip(rows, lens)] if lens is not None
                              else [row for row in rows])
        return self._rows

    @fft_wavelets.setter
    def fft_wavelets(self, rows) -> None:
        freqs = self._cache.freqs if self._cache is not None else np.arange(len(rows), dtype=np.float64)
        self._cache = self._table_cache(list(rows), freqs)
        self._rows = None

    @fft_wavelets.deleter
    def fft_wavelets(self) -> None:
        self._cache = None
        self._rows = None

    # ------------------------------------------------------------------ execution
    def _plan(self, n: int, nsig: int, device: int, scales: tuple[int, int] | None = None,
              slot: int = 0, decim: int = 1, min_batch: int = 1) -> Plan:
        """The cached plan for (n, batch, device, decim) -- of the scale slice [f0, f1) when
        ``scales`` is given (scale-sharded multi-device calls).  ``slot`` is the shard
        index of a multi-device call: a plan is not reentrant, so ``devices=[0, 0]`` gets
        one plan per shard, never one plan driven from two host threads."""
        c = self._cache
        f0, f1 = scales if scales is not None else (0, len(c.freqs))
        nf = f1 - f0
        esz = self.dtype.itemsize
        per_sig = nf * n * esz * 5 + n * esz * 3
        cap = max(1, CHUNK_BYTES // per_sig)
        batch = 1
        while batch < min(nsig, cap):
            batch *= 2
        batch = max(min(batch, cap), min_batch)     # (pair reductions: a chunk holds batch // 2 pairs)
        key = (n, nf, self.dtype.str, bool(self.interpolate), device, batch, self.engine, f0, slot, decim)
        plan = self._plans.get(key)
        if plan is None:
            plan = Plan(n, nf, self.dtype, device, batch, self.interpolate, self.engine, decim=decim)
            self._plans[key] = plan
        self._plans.move_to_end(key)
        if plan.wavelet_token != c.version:
            sl = slice(f0, f1)
            plan.set_wavelet(c.kind, c.params, c.freqs[sl], c.grid,
                             None if c.table is None else c.table[sl], token=c.version,
                             row_len=None if c.row_len is None else c.row_len[sl])
        return plan

    def plan_cache_device_bytes(self) -> int:
        """Device bytes held by the cached plans (sum of nw_stats.device_bytes)."""
        return sum(p.stats()['device_bytes'] for p in self._plans.values())

    def _evict_plans(self, keep: int) -> None:
        """Destroy least-recently-used plans (freeing their device buffers) while the cache
        holds more than ``plan_cache_bytes``; the ``keep`` most recent (this call's) stay."""
        sizes = {k: p.stats()['device_bytes'] for k, p in self._plans.items()}
        total = sum(sizes.values())
        while total > self.plan_cache_bytes and len(self._plans) > keep:
            k, p = self._plans.popitem(last=False)
            total -= sizes[k]
            p.close()

    def _device_decim(self, n: int, decim: int) -> bool:
        """Whether the plans decimate by ``decim`` themselves (nw_plan_set_decim); elsewhere the
        full device result is sliced."""
        if decim == 1 or self.engine == 'rocfft':
            return False
        return L.decim_supported(n, L.NW_F32 if self.dtype == np.float32 else L.NW_F64, decim)

    def _run(self, x: np.ndarray, out_kind: str, decim: int = 1) -> np.ndarray:
        """x: (..., n) signals -> (..., F, ceil(n / decim)) on the device(s); the plan cache is
        trimmed to ``plan_cache_bytes`` after the call (its buffers grow during the call)."""
        self._used = 1
        try:
            if self._device_decim(x.shape[-1], decim):
                return self._run_plans(x, out_kind, decim)
            out = self._run_plans(x, out_kind)
            return out if decim == 1 else np.ascontiguousarray(out[..., ::decim])
        finally:
            if len(self._plans) > 1:
                self._evict_plans(keep=max(1, self._used))

    def _run_plans(self, x: np.ndarray, out_kind: str, decim: int = 1) -> np.ndarray:
        """Several devices shard the signals, or -- with fewer signals than devices (one
        long signal) -- the scales."""
        n = x.shape[-1]
        nsig = int(np.prod(x.shape[:-1])) if x.ndim > 1 else 1
        devs = self.devices or [self.device]
        nf = len(self._cache.freqs)
        if len(devs) > 1 and nsig < len(devs) and nf >= len(devs):
            from .dist import shard
            plans = [self._plan(n, nsig, d, shard(nf, i, len(devs)), slot=i, decim=decim)
                     for i, d in enumerate(devs)]
            self._used = len(plans)
            out = execute_multi(plans, x.reshape(nsig, n), out_kind, shard='scales')
            if out_kind in REDUCTIONS:
                return out
            return out.reshape(x.shape[:-1] + out.shape[-2:])
        if len(devs) > 1 and nsig > 1:
            per = -(-nsig // len(devs))          # the largest balanced block (dist.shard)
            plans = [self._plan(n, per, d, slot=i, decim=decim) for i, d in enumerate(devs)]
            self._used = len(plans)
            out = execute_multi(plans, x.reshape(nsig, n), out_kind)
            if out_kind in REDUCTIONS:
                return out
            return out.reshape(x.shape[:-1] + out.shape[-2:])
        self._used = 1
        return self._plan(n, nsig, devs[0], decim=decim).execute(x, out_kind=out_kind)

    def _broadcast_quirk(self, wave: np.ndarray, out_kind: str) -> np.ndarray:
        """2-D (1, N) input: the reference pads the rows to wave.shape[0] = 1 and
        broadcasts that single bin over fft(wave, axis=-1) (base.py:396-406)."""
        n = wave.shape[1]
        c = self._cache
        nf = len(c.freqs)
        odt = np.complex128 if self.dtype == np.float64 else np.complex64
        if self.interpolate:
            # interpolate_alias on a (1, N) spectrum pads BOTH axes by [0, 1] with zeros
            out = np.zeros((nf, n + 1), dtype=odt)
            return out if out_kind == 'cwt' else np.abs(out) ** (2 if out_kind == 'power' else 1)
        first = np.array([pad_to(np.asarray(r), np.zeros(1))[0] for r in self.fft_wavelets],
                         dtype=np.complex128)
        table = np.repeat(first[:, None], n, axis=1)
        saved = self._cache
        self._cache = _Cache('table', [], c.freqs, L.nw_grid(1.0, n, n), table)
        try:
            return self._run(np.ascontiguousarray(wave[0]), out_kind)
        finally:
            self._cache = saved

    def _transform(self, wave, freqs, reuse: bool, out_kind: str, decim=1) -> np.ndarray:
        decim = check_decim(decim)
        wave = np.asarray(wave)
        if (not reuse) or self._cache is None:
            self._build_cache(freqs, wave.shape[0] / self.sfreq)
        if wave.ndim == 1:
            return self._run(wave, out_kind, decim)
        if wave.ndim == 2 and wave.shape[0] == 1:
            out = self._broadcast_quirk(wave, out_kind)
            return out if decim == 1 else np.ascontiguousarray(out[..., ::decim])
        raise ValueError(f'cwt takes one 1-D signal (or the (1, N) form); got shape {wave.shape}. '
                         'Use cwt_batch for batches of signals.')

    def cwt(self, wave: np.ndarray, freqs, reuse: bool = True, decim: int = 1) -> np.ndarray:
        """Complex CWT (F, N) of one signal (base.py:378-407).  ``decim`` (not in the reference's
        cwt; MNE's decim, as MorseMNE.cwt passes it, wavelets.py:170-191) keeps every decim-th
        sample: exactly ``cwt(...)[..., ::decim]``, (F, ceil(N / decim)), computed at that size
        on the device where ``L.decim_supported`` and sliced from the full device result
        elsewhere.  The wavelet cache is built from the full length either way."""
        return self._transform(wave, freqs, reuse, 'cwt', decim)

    def power(self, wave: np.ndarray, freqs=None, reuse: bool = True, decim: int = 1) -> np.ndarray:
        """|cwt|^2 (base.py:409-425), fused on the device; ``decim`` as in cwt."""
        return self._transform(wave, freqs, reuse, 'power', decim)

    def abs(self, wave: np.ndarray, freqs=None, reuse: bool = True, decim: int = 1) -> np.ndarray:
        """|cwt| (base.py:427-443), fused on the device; ``decim`` as in cwt."""
        return self._transform(wave, freqs, reuse, 'abs', decim)

    def cwt_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True,
                  out: str = 'cwt', decim: int = 1) -> np.ndarray:
        """Batched CWT of (..., N) signals -> (..., F, N) in one device call, or (F, N)
        for the reductions over all signals: ``power_mean``, ``itc`` (the compute
        dtype), ``power_sum`` (float64) and ``phase_sum`` (complex128).

        Equivalent to stacking ``cwt(w, freqs, reuse)`` over the leading axes
        (the per-epoch loop of mneutils.py:39): the cache is built from the
        first call's length if absent, then shared by every signal.  ``decim`` as in cwt:
        the last axis holds the samples ``[..., ::decim]`` of the undecimated result."""
        decim = check_decim(decim)
        waves = np.asarray(waves)
        if waves.ndim < 1:
            raise ValueError('waves must have a trailing sample axis')
        if (not reuse) or self._cache is None:
            self._build_cache(freqs, waves.shape[-1] / self.sfreq)
        if out not in ('cwt', 'abs', 'power') + REDUCTIONS:
            raise ValueError(f"out must be one of cwt, abs, power, {', '.join(REDUCTIONS)}; got {out!r}")
        return self._run(waves, out, decim)

    def cross_batch(self, waves_a: np.ndarray, waves_b: np.ndarray, freqs=None, reuse: bool = True,
                    out: str = 'coherence', decim: int = 1) -> np.ndarray:
        """Cross-channel reduction over the signal pairs (waves_a[e], waves_b[e]) of two (..., N)
        arrays of equal shape (the epochs of two channels), reduced on the device in fp64 in
        pair order: the (E, F, N) CWTs are never materialised (no reference counterpart; the
        cache semantics are cwt_batch's).  With y_a, y_b the CWT rows of a pair,
        S_ab = sum_e y_a conj(y_b), P_aa = sum_e |y_a|^2 and E pairs, ``out`` is one of
          cross_sum  float64 (F, N, 4) = {Re S_ab, Im S_ab, P_aa, P_bb}
          plv_sum    complex128 (F, N) = sum_e (y_a / |y_a|) conj(y_b / |y_b|)
          csd        S_ab / E              coherency  S_ab / sqrt(P_aa P_bb)   (complex128)
          coherence  |coherency|           imcoh      Im coherency             (float64)
          plv        |plv_sum| / E  (float64; NaN where some |y| = 0, as itc)
        (engine.finalize_pair).  Results are float64 / complex128 whatever the compute dtype.
        One device is used: the first of the wavelet's.  ``decim`` as in cwt."""
        return self._pair_sums(waves_a, waves_b, freqs, reuse, out, decim, PAIR_OUTS, finalize_pair, 0)

    def _pair_sums(self, waves_a, waves_b, freqs, reuse, out, decim, names, finalize, min_pairs):
        """The measures of the signal pairs of two (..., N) arrays: the argument checks (``out`` one of
        ``names``, equal shapes, at least ``min_pairs`` pairs), sums = plan.execute_pair over the pairs
        (_sums_on_plan; the plan holds max_batch >= 2, one pair) and finalize(out, sums, npairs)."""
        decim = check_decim(decim)
        if out not in names:
            raise ValueError(f"out must be one of {', '.join(names)}; got {out!r}")
        waves_a, waves_b = np.asarray(waves_a), np.asarray(waves_b)
        if waves_a.ndim < 1 or waves_a.shape != waves_b.shape:
            raise ValueError(f'waves_a and waves_b must have the same (..., N) shape; got {waves_a.shape} '
                             f'and {waves_b.shape}')
        n = waves_a.shape[-1]
        npairs = int(np.prod(waves_a.shape[:-1])) if waves_a.ndim > 1 else 1
        if npairs < min_pairs:
            raise ValueError(f'{out} needs at least {min_pairs} epochs, got {npairs}')
        sums = self._sums_on_plan(freqs, reuse, n, 2 * npairs, decim, 2, 1, lambda plan: plan.execute_pair(
            waves_a.reshape(npairs, n), waves_b.reshape(npairs, n), out_kind=names[out]))
        return finalize(out, sums, npairs)

    def _conn_sums(self, waves, freqs, reuse, out, indices, decim, names, finalize, min_epochs):
        """_pair_sums for the channel pairs ``indices`` of (E, C, N) epochs: sums = plan.execute_conn (the
        plan holds max_batch >= C, one epoch) and finalize(sums, ia, ib, E)."""
        decim = check_decim(decim)
        if out not in names:
            raise ValueError(f"out must be one of {', '.join(names)}; got {out!r}")
        waves, nep, nchan, n = _epochs(waves)
        pairs = check_indices(indices, nchan)
        if nep < min_epochs:
            raise ValueError(f'{out} needs at least {min_epochs} epochs, got {nep}')
        sums = self._sums_on_plan(freqs, reuse, n, nep * nchan, decim, nchan, 2,
                                  lambda plan: plan.execute_conn(waves, pairs, out_kind=names[out]))
        return finalize(sums, *pairs, nep)

    def _sums_on_plan(self, freqs, reuse, n, nsig, decim, min_batch, axis, execute):
        """The epoch sums execute(plan) (one array or a tuple of them, samples on ``axis``) at every
        ``decim``-th sample: the cache, then the plan of _on_plan, which decimates where the device can;
        elsewhere the full-rate sums are sliced."""
        if (not reuse) or self._cache is None:
            self._build_cache(freqs, n / self.sfreq)
        on_device = self._device_decim(n, decim)
        sums = self._on_plan(n, nsig, decim if on_device else 1, min_batch, execute)
        if decim == 1 or on_device:
            return sums
        every = (slice(None),) * axis + (slice(None, None, decim),)
        if isinstance(sums, tuple):
            return tuple(np.ascontiguousarray(s[every]) for s in sums)
        return np.ascontiguousarray(sums[every])

    def connectivity_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, out: str = 'coherence',
                           indices=None, decim: int = 1):
        """Connectivity between the channels of ``waves`` (E, C, N), E epochs of C channels: every
        signal is transformed ONCE and the sums of cross_batch are formed on the device for all
        pairs ``indices`` = (ia, ib) (positions on the channel axis; any list: repeats, a > b,
        a == b; default every pair a < b in np.triu_indices(C, 1) order) -- C E transforms where
        one cross_batch call per pair takes C (C - 1) E.  The result is (P, F, ceil(N / decim)) with
        ``out`` as in cross_batch (csd, coherency: complex128; coherence, imcoh, plv: float64;
        plv_sum: complex128), each pair finalised as cross_batch finalises it; ``cross_sum``
        returns (S complex128 (P, F, N'), P_cc float64 (C, F, N')).  No reference counterpart
        (mne-connectivity's spectral_connectivity_epochs(..., indices=...) in its cwt_morlet mode
        returns the same maps); cache semantics, device choice and ``decim`` as in cross_batch."""
        def finalize(sums, *a):
            return finalize_conn(out, *(sums if CONN_OUTS[out] == 'cross_sum' else (sums, None)), *a)
        return self._conn_sums(waves, freqs, reuse, out, indices, decim, CONN_OUTS, finalize, 0)

    def lag_batch(self, waves_a: np.ndarray, waves_b: np.ndarray, freqs=None, reuse: bool = True,
                  out: str = 'wpli', decim: int = 1) -> np.ndarray:
        """Phase-lag connectivity of the signal pairs (waves_a[e], waves_b[e]), (F, N'): cross_batch
        for the measures that ignore zero-lag coupling (mne-connectivity's names).  With
        m_e = Im y_a conj(y_b) of pair e, the device forms {L0, L1, L2, L3} = the sums over e of
        m, |m|, m^2, sgn m in fp64 in pair order, and ``out`` is one of
          lag_sum         float64 (F, N', 4), the sums themselves
          pli             |L3| / E                  dpli            0.5 + 0.5 L3 / E
          pli2_unbiased   (E pli^2 - 1) / (E - 1)   wpli            |L0| / L1
          wpli2_debiased  (L0^2 - L2) / (L1^2 - L2)
          ciplv, ppc      from cross_batch's plv_sum
        (engine.finalize_lag; float64).  Argument checks, cache semantics, device choice and
        ``decim`` as in cross_batch."""
        return self._pair_sums(waves_a, waves_b, freqs, reuse, out, decim, LAG_OUTS, finalize_lag,
                               2 if out in ('pli2_unbiased', 'ppc') else 0)

    def lag_connectivity_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, out: str = 'wpli',
                               indices=None, decim: int = 1) -> np.ndarray:
        """lag_batch's measures for the channel pairs ``indices`` of ``waves`` (E, C, N) from ONE
        transform per epoch and channel, (P, F, N') float64 (``lag_sum``: (P, F, N', 4)), as
        connectivity_batch does for the cross sums: its argument checks, pair lists, cache
        semantics, device choice and ``decim``."""
        return self._conn_sums(waves, freqs, reuse, out, indices, decim, LAG_OUTS,
                               lambda sums, ia, ib, nep: finalize_lag(out, sums, nep),
                               2 if out in ('pli2_unbiased', 'ppc') else 0)

    def connectivity_time_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, out: str = 'coherence',
                                indices=None, window=None, decim: int = 1, average: bool = False):
        """Over-time connectivity of ``waves`` (E, C, N): connectivity_batch's and
        lag_connectivity_batch's measures with every sum taken over the SAMPLES of an epoch instead
        of over the epochs, one value per epoch, pair and scale: (E, P, F) (what mne-connectivity's
        spectral_connectivity_time returns per epoch).  Every signal is transformed once and reduced
        on the device; the (E, C, F, N) rows never leave it.  ``out``: any name of CONN_OUTS or
        LAG_OUTS (engine.finalize_conn_time, the sample count T in the place of the epoch count;
        ``cross_sum`` returns (S (E, P, F), P_cc (E, C, F)), ``lag_sum`` (E, P, F, 4)).  ``window`` =
        (t0, t1) in full-rate samples (None: the whole epoch); with ``decim`` the samples summed are
        the decimated samples j * decim in [t0, t1).  ``average=True``: the mean over the epochs of
        the finalised measure, (P, F) (ValueError for the ``*_sum`` kinds).  pli2_unbiased and ppc
        need T >= 2.  Pair lists, cache semantics, device choice and plan eviction as in
        connectivity_batch."""
        outs = {**CONN_OUTS, **LAG_OUTS}

        def finalize(sums, *a):
            return finalize_conn_time(out, *(sums if outs[out] == 'cross_sum' else (sums, None)), *a)
        return self._time_sums(waves, freqs, reuse, out, outs, check_indices, indices, window, decim, average,
                               2 if out in ('pli2_unbiased', 'ppc') else 0,
                               lambda plan, *a: plan.execute_conn_time(*a, out_kind=outs[out]), finalize)

    def _time_sums(self, waves, freqs, reuse, out, names, check_pairs, indices, window, decim, average, min_count,
                   execute, finalize, scales=None, min_epochs=0):
        """The over-time measures of (E, C, N) epochs: the argument checks (``out`` one of ``names``,
        the pair list by ``check_pairs``, at least ``min_count`` window samples and ``min_epochs`` epochs;
        ``scales``: pac_batch's (phase, amp) lists), the cache, the plan of the first device with max_batch >= C and its
        eviction, sums = execute(plan, waves, pairs, *scales, window, step) and
        finalize(sums, *pairs, count), averaged over the epochs where asked."""
        decim = check_decim(decim)
        if out not in names:
            raise ValueError(f"out must be one of {', '.join(names)}; got {out!r}")
        if average and out.endswith('_sum'):
            raise ValueError(f'average=True takes a finalised measure, not the sums {out!r}')
        waves, nep, nchan, n = _epochs(waves)
        pairs = check_pairs(indices, nchan)
        if nep < min_epochs:
            raise ValueError(f'{out} needs at least {min_epochs} epochs, got {nep}')
        rebuild = (not reuse) or self._cache is None
        if scales is not None:
            nfreq = len(list(freqs)) if rebuild else len(self._cache.freqs)     # the scale list the call will use
            scales = check_scales('phase', scales[0], nfreq), check_scales('amp', scales[1], nfreq)
        count = time_window(n, decim, window, False)[3]     # the same count on either kind of plan
        if count < min_count:
            raise ValueError(f'{out} needs at least {min_count} sample{"s" if min_count > 1 else ""} in the window, '
                             f'got {count}')
        if rebuild:
            self._build_cache(freqs, n / self.sfreq)
        on_device = self._device_decim(n, decim)
        t0, t1, step, count = time_window(n, decim, window, on_device)
        sums = self._on_plan(n, nep * nchan, decim if on_device else 1, nchan,
                             lambda plan: execute(plan, waves, pairs, *(scales or ()), (t0, t1), step))
        res = finalize(sums, *pairs, count)
        return res.mean(axis=0) if average else res

    def _on_plan(self, n, nsig, decim, min_batch, call):
        """call(plan) on the first device's plan for nsig signals (max_batch >= min_batch); the other
        plans are evicted afterwards."""
        self._used = 1
        try:
            return call(self._plan(n, nsig, (self.devices or [self.device])[0], decim=decim, min_batch=min_batch))
        finally:
            if len(self._plans) > 1:
                self._evict_plans(keep=1)

    def envelope_correlation_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, out: str = 'aec_orth',
                                   indices=None, window=None, decim: int = 1, average: bool = False):
        """Envelope correlation of ``waves`` (E, C, N) (Hipp et al. 2012; mne-connectivity's
        envelope_correlation): per epoch, pair and scale the Pearson correlation over time of the two
        channels' amplitude envelopes |cwt|, (E, P, F) float64.  Every signal is transformed once and
        reduced on the device; the (E, C, F, N) rows never leave it.  ``out`` (engine.finalize_env):
        ``aec_orth`` (mne's default: each signal orthogonalised against the other sample by sample, so
        that zero-lag field spread gives no correlation; the mean of the two directions' |r|),
        ``aec_orth_signed`` (absolute=False), ``aec_directed`` ((E, P, F, 2): both directions), ``aec``
        (no orthogonalisation); ``env_sum`` / ``env_orth_sum`` return the sums (pair, chan).
        ``window``, ``decim`` and ``average`` (the mean over the epochs, (P, F); ValueError for the
        ``*_sum`` kinds) as in connectivity_time_batch; the finalised kinds need T >= 2 window samples.
        Pair lists, cache semantics, device choice and plan eviction as in connectivity_batch."""
        return self._time_sums(waves, freqs, reuse, out, ENV_OUTS, check_indices, indices, window, decim, average,
                               0 if str(out).endswith('_sum') else 2,
                               lambda plan, *a: plan.execute_env_time(*a, out_kind=ENV_OUTS[out]),
                               lambda sums, *a: finalize_env(out, *sums, *a))

    def pac_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, phase=None, amp=None,
                  out: str = 'direct_pac', indices=None, window=None, decim: int = 1, average: bool = False):
        """Phase-amplitude coupling of ``waves`` (E, C, N): how the amplitude of the scales ``amp``
        follows the phase of the scales ``phase`` (both lists of positions into the scale list; any
        lists), one comodulogram per epoch and pair: (E, P, Fp, Fa) float64.  ``indices`` = (ip, ia),
        the phase and the amplitude channel of each pair (None: every channel with itself, P = C).
        Every signal is transformed once and reduced on the device; the (E, C, F, N) rows never leave
        it.  ``out``: mvl, mvl_norm, direct_pac or debiased_pac (engine.finalize_pac); ``pac_sum``
        returns the sums (M (E, P, Fp, Fa), amp (E, C, Fa, 2), phase (E, C, Fp)).  ``window``, ``decim``
        and ``average`` (the mean over the epochs, (P, Fp, Fa); ValueError for ``pac_sum``) as in
        connectivity_time_batch; an empty window is a ValueError for the finalised kinds.  Cache
        semantics, device choice and plan eviction as in connectivity_batch."""
        return self._time_sums(waves, freqs, reuse, out, dict.fromkeys(sorted(PAC_OUTS)), check_pac_indices, indices,
                               window, decim, average, 0 if out == 'pac_sum' else 1,
                               lambda plan, *a: plan.execute_pac(*a),
                               lambda sums, *a: finalize_pac(out, *sums, *a), scales=(phase, amp))

    def pac_surrogates_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, phase=None, amp=None,
                             out: str = 'direct_pac', stat: str = 'zscore', n_surrogates: int = 200, lags=None,
                             min_lag=None, seed=None, indices=None, window=None, decim: int = 1, average: bool = False):
        """Whether pac_batch's coupling is above chance: time-lag surrogates (Canolty et al. 2006; tensorpac's
        "swap amplitude time blocks").  The amplitude of every epoch is cut at a random sample of the window and
        its two blocks are swapped -- a circular shift -- which keeps both signals' spectra and breaks their
        timing; the measure ``out`` (mvl, mvl_norm, direct_pac, debiased_pac) is formed again for every shift, all
        on the device from ONE transform per epoch and channel.  ``stat`` (engine.finalize_pac_surr): ``zscore``
        (the observed value against the surrogates' mean and sd), ``pvalue`` ((1 + #{surrogate >= observed}) /
        (1 + S)), ``surr_mean``, ``surr_std``, ``surr_max`` (in the measure's units), each (E, P, Fp, Fa) float64;
        ``surrogates``: every surrogate value, (E, P, Fp, Fa, S); ``surr_sum``: the sums (M, amp, phase, stat, None).
        ``lags``: the shifts in window samples, integers in [0, T) (at most NW_PAC_MAX_LAGS; the same list for
        every epoch, pair and cell); None: default_rng(``seed``).integers(min_lag, T - min_lag + 1,
        ``n_surrogates``) with ``min_lag`` = max(1, T // 10) unless given (ValueError if T < 2 min_lag).
        ``phase``, ``amp``, ``indices``, ``window`` and ``decim`` as in pac_batch (T: the window's decimated
        samples); ``average=True``: the mean over the epochs of zscore, surr_mean or surr_std, (P, Fp, Fa)
        (ValueError for the other kinds).  zscore and surr_std need at least 2 surrogates.  A strictly periodic
        driver keeps its coupling under a shift: its z is small by construction.  Cache semantics, device choice
        and plan eviction as in connectivity_batch."""
        kinds = dict.fromkeys(sorted(PAC_OUTS - {'pac_sum'}))
        if stat not in PAC_SURR_STATS:
            raise ValueError(f"stat must be one of {', '.join(sorted(PAC_SURR_STATS))}; got {stat!r}")
        if average and stat not in ('zscore', 'surr_mean', 'surr_std'):
            raise ValueError(f'average=True takes zscore, surr_mean or surr_std, not {stat!r}')
        if out not in kinds:
            raise ValueError(f"out must be one of {', '.join(kinds)}; got {out!r}")
        _, _, _, n = _epochs(waves)
        T = time_window(n, check_decim(decim), window, False)[3]
        if T < 1:
            raise ValueError(f'{stat} needs at least 1 sample in the window, got {T}')
        lags = draw_lags(T, n_surrogates, min_lag, seed) if lags is None else check_lags(lags, T)
        need = 2 if stat in ('zscore', 'surr_std') else 0 if stat == 'surr_sum' else 1
        if lags.size < need:
            raise ValueError(f'{stat} needs at least {need} surrogate{"s" if need > 1 else ""}, got {lags.size}')
        centre = 'debiased' if out == 'debiased_pac' else 'plain'
        keep = stat == 'surrogates'
        return self._time_sums(waves, freqs, reuse, out, kinds, check_pac_indices, indices, window, decim, average, 1,
                               lambda plan, *a: plan.execute_pac_surr(a[0], lags, *a[1:], centre=centre, keep_all=keep),
                               lambda sums, ip, ia, count: finalize_pac_surr(out, stat, *sums[:4], sums[4] if keep else None,
                                                                             ip, ia, count, lags.size),
                               scales=(phase, amp))

    def erpac_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, phase=None, amp=None,
                    out: str = 'circular', indices=None, window=None, decim: int = 1):
        """Event-related phase-amplitude coupling of ``waves`` (E, C, N) (ERPAC; Voytek et al. 2013): WHEN,
        relative to the event the epochs are locked to, the amplitude of the scales ``amp`` follows the phase
        of the scales ``phase`` -- the coupling is formed ACROSS the epochs at every sample, one time course
        per pair and (phase scale, amplitude scale): (P, Fp, Fa, N') float64.  Every signal is transformed once
        and reduced on the device; the (E, C, F, N) rows never leave it.  ``out`` (engine.finalize_erpac):
        ``circular`` (the circular-linear correlation of phase and amplitude over the epochs, tensorpac's
        EventRelatedPac(method='circular')), ``circular_pval`` (its p-value), and pac_batch's mvl, mvl_norm,
        direct_pac and debiased_pac taken over the epochs; ``erpac_sum`` returns the sums (M (P, Fp, Fa, N'), amp
        (C, Fa, N', 2), phase (C, Fp, 5, N')).  ``phase``, ``amp`` and ``indices`` as in pac_batch; ``window`` =
        (t0, t1) in full-rate samples (None: the whole epoch) and ``decim`` as in connectivity_time_batch: N' is
        the number of decimated samples j * decim in [t0, t1).  The circular kinds need E >= 2, the others
        E >= 1.  There is no ``average``: the epochs are already reduced.  The plan takes as many epochs per
        chunk as the plan-size policy allows: the device reads and writes its (P, Fp, Fa, N') accumulators once
        per chunk, so the rate depends on the epochs per chunk.  Cache semantics, device choice
        and plan eviction as in connectivity_batch."""
        need = 0 if out == 'erpac_sum' else 2 if str(out).startswith('circular') else 1
        return self._time_sums(waves, freqs, reuse, out, dict.fromkeys(sorted(ERPAC_OUTS)), check_pac_indices, indices,
                               window, decim, False, 0, lambda plan, *a: plan.execute_erpac(*a),
                               lambda sums, ip, ia, count: finalize_erpac(out, *sums, ip, ia, len(waves)),
                               scales=(phase, amp), min_epochs=need)

    def pac_bins_batch(self, waves: np.ndarray, freqs=None, reuse: bool = True, phase=None, amp=None, out: str = 'mi',
                       nbins: int = 18, indices=None, window=None, decim: int = 1, average: bool = False):
        """Phase-binned phase-amplitude coupling of ``waves`` (E, C, N): the amplitude of the scales ``amp``
        averaged within ``nbins`` bins of the phase of the scales ``phase``, and what is formed from that
        distribution (engine.finalize_pac_bins): ``mi`` (Tort's Kullback-Leibler modulation index, tensorpac's
        idpac=(2, ...)), ``hr`` (the height ratio) and ``pref_phase`` (the centre of the bin with the largest
        mean amplitude), each (E, P, Fp, Fa) float64, and ``bin_amp``, the phase-amplitude histogram
        (E, P, Fp, Fa, nbins); ``bin_sum`` returns the sums (S (E, P, Fp, Fa, nbins), count (E, C, Fp, nbins)).
        ``nbins`` even, 2 .. 36.  Every signal is transformed once and reduced on the device; the (E, C, F, N)
        rows never leave it.  ``phase``, ``amp``, ``indices``, ``window``, ``decim`` and ``average`` (the mean over
        the epochs; ValueError for ``bin_sum`` and for ``pref_phase``, an angle) as in pac_batch; an empty
        window is a ValueError for the finalised kinds.  Cache semantics, device choice and plan eviction
        as in connectivity_batch."""
        nbins = check_nbins(nbins)
        if average and out == 'pref_phase':
            raise ValueError("average=True takes a measure that can be averaged over the epochs, not the angle 'pref_phase'")
        return self._time_sums(waves, freqs, reuse, out, dict.fromkeys(sorted(PAC_BIN_OUTS)), check_pac_indices, indices,
                               window, decim, average, 0 if out == 'bin_sum' else 1,
                               lambda plan, *a: plan.execute_pac_bins(*a, nbins=nbins),
                               lambda sums, ip, ia, count: finalize_pac_bins(out, *sums, ip), scales=(phase, amp))

    def plan_stats(self) -> list:
        """Per-plan device stage timings (nw_plan_stats)."""
        return [p.stats() for p in self._plans.values()]
