"""Thin Python owner of one ``nw_plan`` (one device, one signal length n).

This is the batched entry point that replaces the serial per-epoch loop of
the reference (mneutils.py:39): one call transforms S = epochs x channels
signals.  Inputs/outputs may be numpy arrays (host, synchronous) or device
buffers (torch tensors on the plan's device or raw pointers; asynchronous on
the plan stream).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

from . import _lib as L

OUT_KINDS = {'cwt': L.NW_OUT_CWT, 'abs': L.NW_OUT_ABS, 'power': L.NW_OUT_POWER,
             # reductions over the signals -> (F, n) (EpochsWavelet, mneutils.py:42-71)
             'power_mean': L.NW_OUT_POWER_MEAN, 'itc': L.NW_OUT_ITC,
             'power_sum': L.NW_OUT_POWER_SUM, 'phase_sum': L.NW_OUT_PHASE_SUM}
REDUCTIONS = ('power_mean', 'itc', 'power_sum', 'phase_sum')
# cross-channel reductions over signal pairs -> (F, n, 4) float64 / (F, n) complex128 (Plan.execute_pair)
PAIR_KINDS = {'cross_sum': L.NW_OUT_CROSS_SUM, 'plv_sum': L.NW_OUT_PLV_SUM}
# what finalize_pair forms from them: name -> the sums it needs
PAIR_OUTS = {'cross_sum': 'cross_sum', 'plv_sum': 'plv_sum', 'csd': 'cross_sum', 'coherency': 'cross_sum',
             'coherence': 'cross_sum', 'imcoh': 'cross_sum', 'plv': 'plv_sum'}
# multi-channel connectivity (Plan.execute_conn): the same two sums for every channel pair of a list,
# cross_sum -> complex128 (P, F, n) + float64 (C, F, n), plv_sum -> complex128 (P, F, n); and what
# finalize_conn forms from them
CONN_KINDS, CONN_OUTS = PAIR_KINDS, PAIR_OUTS
# phase-lag connectivity (Plan.execute_pair / execute_conn with out_kind='lag_sum'): float64
# (..., 4) = {L0, L1, L2, L3}, the epoch sums of m, |m|, m^2, sgn m with m = Im y_a conj(y_b); and
# what finalize_lag forms, name -> the sums it needs (ciplv and ppc come from the unit-phasor sums)
LAG_KINDS = {'lag_sum': L.NW_OUT_LAG_SUM}
LAG_OUTS = {'lag_sum': 'lag_sum', 'pli': 'lag_sum', 'pli2_unbiased': 'lag_sum', 'dpli': 'lag_sum',
            'wpli': 'lag_sum', 'wpli2_debiased': 'lag_sum', 'ciplv': 'plv_sum', 'ppc': 'plv_sum'}
# phase-amplitude coupling (Plan.execute_pac): what finalize_pac forms from its sums (M, amp, phase)
PAC_OUTS = {'pac_sum', 'mvl', 'mvl_norm', 'direct_pac', 'debiased_pac'}
# time-lag surrogates (Plan.execute_pac_surr): what finalize_pac_surr forms from its sums for a measure of PAC_OUTS
PAC_SURR_STATS = {'surr_sum', 'zscore', 'pvalue', 'surr_mean', 'surr_std', 'surr_max', 'surrogates'}
PAC_SURR_CENTRES = {'plain': L.NW_PAC_SURR_PLAIN, 'debiased': L.NW_PAC_SURR_DEBIASED}
# event-related coupling (Plan.execute_erpac): what finalize_erpac forms from its across-epoch sums (M, amp, phase)
ERPAC_OUTS = {'erpac_sum', 'circular', 'circular_pval', 'mvl', 'mvl_norm', 'direct_pac', 'debiased_pac'}
# phase-binned coupling (Plan.execute_pac_bins): what finalize_pac_bins forms from its sums (S, count)
PAC_BIN_OUTS = {'bin_sum', 'bin_amp', 'mi', 'hr', 'pref_phase'}
# envelope correlation (Plan.execute_env_time): the Pearson sums of two amplitude envelopes, plain
# (float64 (E, P, F)) or pairwise orthogonalised (float64 (E, P, F, 6)), each with the per-channel sums
# float64 (E, C, F, 2); and what finalize_env forms, name -> the sums it needs
ENV_KINDS = {'env_sum': L.NW_ENV_PLAIN, 'env_orth_sum': L.NW_ENV_ORTH}
ENV_OUTS = {'env_sum': 'env_sum', 'env_orth_sum': 'env_orth_sum', 'aec': 'env_sum',
            'aec_directed': 'env_orth_sum', 'aec_orth': 'env_orth_sum', 'aec_orth_signed': 'env_orth_sum'}
KINDS = {'morse': L.NW_MORSE, 'morlet': L.NW_MORLET, 'shannon': L.NW_SHANNON, 'table': L.NW_TABLE,
         # WaveletMode.Normal tables built on the device (base.py:249-256)
         'mexican_hat': L.NW_MEXICAN_HAT, 'haar': L.NW_HAAR}
TABLE_KINDS = ('table', 'mexican_hat', 'haar')


def np_dtype(dtype) -> np.dtype:
    dt = np.dtype(dtype)
    if dt not in (np.float32, np.float64):
        raise ValueError(f'compute dtype must be float32 or float64, got {dt}')
    return dt


def check_decim(decim) -> int:
    """``decim`` as an int >= 1 (MNE's decim, the reference's MorseMNE.cwt, wavelets.py:170-191);
    ValueError for anything else, before any device work."""
    import operator
    try:
        d = operator.index(decim)
    except TypeError:
        raise ValueError(f'decim must be an integer >= 1, got {decim!r}') from None
    if isinstance(decim, bool) or d < 1:
        raise ValueError(f'decim must be an integer >= 1, got {decim!r}')
    return d


def out_dtype(dtype, out_kind: str) -> np.dtype:
    dt = np_dtype(dtype)
    if out_kind == 'power_sum':                 # fp64 partial sums whatever the compute dtype
        return np.dtype(np.float64)
    if out_kind == 'phase_sum':
        return np.dtype(np.complex128)
    if out_kind == 'cwt':
        return np.dtype(np.complex64 if dt == np.float32 else np.complex128)
    return dt


def finalize_pair(kind: str, sums: np.ndarray, npairs: int) -> np.ndarray:
    """The connectivity measure ``kind`` from the fp64 sums over ``npairs`` signal pairs
    (a_e, b_e) that Plan.execute_pair returns.  From ``cross_sum`` (F, n, 4) =
    {Re S_ab, Im S_ab, P_aa, P_bb} with S_ab = sum_e y_a conj(y_b), P_aa = sum_e |y_a|^2:
      csd        S_ab / E                        complex128
      coherency  S_ab / sqrt(P_aa P_bb)          complex128
      coherence  |coherency|                     float64
      imcoh      Im coherency                    float64
    from ``plv_sum`` (F, n) = sum_e (y_a / |y_a|) conj(y_b / |y_b|):
      plv        |plv_sum| / E                   float64
    ``cross_sum`` / ``plv_sum`` return the sums themselves.  Plain numpy, float64 / complex128
    whatever the compute dtype."""
    if kind not in PAIR_OUTS:
        raise ValueError(f"out must be one of {', '.join(PAIR_OUTS)}; got {kind!r}")
    if kind in PAIR_KINDS:
        return sums
    if kind == 'plv':
        return np.abs(np.asarray(sums, dtype=np.complex128)) / npairs
    sums = np.asarray(sums, dtype=np.float64)
    # S_ab over a real: two real divisions (numpy's complex / real is not correctly rounded: the
    # coherence of a channel with itself would come out 1 - 1 ulp)
    den = npairs if kind == 'csd' else np.sqrt(sums[..., 2] * sums[..., 3])
    ratio = np.empty(sums.shape[:-1], dtype=np.complex128)
    ratio.real, ratio.imag = sums[..., 0] / den, sums[..., 1] / den
    if kind in ('csd', 'coherency'):
        return ratio
    return np.abs(ratio) if kind == 'coherence' else np.ascontiguousarray(ratio.imag)


def finalize_lag(kind: str, sums: np.ndarray, nepochs: int) -> np.ndarray:
    """The phase-lag measure ``kind`` (mne-connectivity's spectral_connectivity_epochs names) from
    the fp64 sums over E = ``nepochs`` epochs.  From ``lag_sum`` (..., 4) = {L0, L1, L2, L3}, the
    sums of m, |m|, m^2, sgn m with m = Im y_a conj(y_b):
      pli             |L3| / E
      dpli            0.5 + 0.5 L3 / E        (the mean Heaviside step of m, H(0) = 1/2)
      pli2_unbiased   (E pli^2 - 1) / (E - 1)
      wpli            |L0| / L1                        (0 where L1 = 0)
      wpli2_debiased  (L0^2 - L2) / (L1^2 - L2)        (0 where the denominator is 0)
    from a complex ``plv_sum`` Phi = sum_e (y_a / |y_a|) conj(y_b / |y_b|):
      ciplv           i / sqrt(1 - r^2), r = clip(Re Phi / E, -1, 1), i = |Im Phi| / E  (i where |r| = 1)
      ppc             (|Phi|^2 - E) / (E (E - 1))
    ``lag_sum`` returns the sums themselves.  Plain numpy, float64, any leading shape;
    pli2_unbiased and ppc need E >= 2 (ValueError)."""
    if kind not in LAG_OUTS:
        raise ValueError(f"out must be one of {', '.join(LAG_OUTS)}; got {kind!r}")
    if kind == 'lag_sum':
        return sums
    E = int(nepochs)
    if kind in ('pli2_unbiased', 'ppc') and E < 2:
        raise ValueError(f'{kind} needs at least 2 epochs, got {E}')
    if LAG_OUTS[kind] == 'plv_sum':
        phi = np.asarray(sums, dtype=np.complex128)
        if kind == 'ppc':
            return (phi.real * phi.real + phi.imag * phi.imag - E) / (E * (E - 1))
        r, i = np.clip(phi.real / E, -1., 1.), np.abs(phi.imag) / E
        den = np.sqrt(1. - r * r)
        edge = den == 0
        return np.where(edge, i, i / np.where(edge, 1., den))
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim < 1 or sums.shape[-1] != 4:
        raise ValueError(f'lag sums must be (..., 4), got shape {sums.shape}')
    l0, l1, l2, l3 = (sums[..., j] for j in range(4))
    if kind == 'dpli':
        return 0.5 + 0.5 * l3 / E
    if kind in ('pli', 'pli2_unbiased'):
        pli = np.abs(l3) / E
        return pli if kind == 'pli' else (E * pli * pli - 1.) / (E - 1)
    num, den = (np.abs(l0), l1) if kind == 'wpli' else (l0 * l0 - l2, l1 * l1 - l2)
    zero = den == 0
    return np.where(zero, 0., num / np.where(zero, 1., den))


def all_pairs(nchan: int):
    """(ia, ib), int32: every channel pair a < b of ``nchan`` channels in np.triu_indices(nchan, 1)
    order, the default pair list of the connectivity calls."""
    ia, ib = np.triu_indices(int(nchan), 1)
    return ia.astype(np.int32), ib.astype(np.int32)


def check_indices(indices, nchan: int):
    """``indices`` = (ia, ib), two equally long 1-D lists of channel positions in [0, nchan)
    (None: all_pairs(nchan)), as contiguous int32 arrays; ValueError otherwise.  Any list is
    allowed: repeated pairs, a > b, a == b."""
    if indices is None:
        return all_pairs(nchan)
    try:
        ia, ib = indices
        ia, ib = np.asarray(ia), np.asarray(ib)
    except (TypeError, ValueError):
        raise ValueError('indices must be a pair (ia, ib) of index lists') from None
    if ia.ndim != 1 or ib.ndim != 1 or ia.shape != ib.shape:
        raise ValueError(f'indices must be two 1-D lists of equal length, got shapes {ia.shape} and {ib.shape}')
    if ia.size and not (np.issubdtype(ia.dtype, np.integer) and np.issubdtype(ib.dtype, np.integer)):
        raise ValueError(f'indices must be integers, got {ia.dtype} and {ib.dtype}')
    if ia.size and (min(ia.min(), ib.min()) < 0 or max(ia.max(), ib.max()) >= nchan):
        raise ValueError(f'indices must lie in [0, {nchan}): got {int(min(ia.min(), ib.min()))} .. '
                         f'{int(max(ia.max(), ib.max()))}')
    return np.ascontiguousarray(ia, dtype=np.int32), np.ascontiguousarray(ib, dtype=np.int32)


def finalize_conn(kind: str, cross: np.ndarray, power, ia, ib, nepochs: int):
    """The connectivity measure ``kind`` of every pair p = (ia[p], ib[p]) from the sums over
    ``nepochs`` epochs that Plan.execute_conn returns: ``cross`` complex128 (P, F, n) = S_p (for
    ``plv`` / ``plv_sum``: Phi_p) and ``power`` float64 (C, F, n) = P_cc (unused, may be None, for
    the two plv kinds).  finalize_pair is applied pair by pair to stack(Re S, Im S, P_aa, P_bb), so
    the rounding is that of the two-channel calls (the coherence of a channel with itself is
    exactly 1) and only one pair's intermediate arrays exist at a time.  ``cross_sum`` returns
    (cross, power) and ``plv_sum`` returns cross; the others (P, F, n): csd and coherency
    complex128, coherence, imcoh and plv float64."""
    if kind not in CONN_OUTS:
        raise ValueError(f"out must be one of {', '.join(CONN_OUTS)}; got {kind!r}")
    if kind == 'cross_sum':
        return cross, power
    if kind == 'plv_sum':
        return cross
    return _finalize_pairs(kind, cross, power, ia, ib, nepochs, 0)


def _finalize_pairs(kind: str, sums, power, ia, ib, count: int, axis: int):
    """The per-pair loop of finalize_conn (pairs and channels on axis 0) and finalize_conn_time (on
    ``axis`` 1): pair p's slice of ``sums`` through finalize_lag, or finalize_pair on it (plv) or on
    stack(Re S, Im S, P of ia[p], P of ib[p]), into pair p's slice of a result of sums' layout."""
    lag = kind in LAG_OUTS
    sums = np.asarray(sums) if lag else np.asarray(sums, dtype=np.complex128)
    out = np.empty(sums.shape[:-1] if LAG_OUTS.get(kind) == 'lag_sum' else sums.shape,
                   dtype=np.complex128 if kind in ('csd', 'coherency') else np.float64)
    rows, res = np.moveaxis(sums, axis, 0), np.moveaxis(out, axis, 0)          # views, pair axis first
    chan = None if lag or kind == 'plv' else np.moveaxis(power, axis, 0)
    for p in range(rows.shape[0]):
        if lag:
            res[p] = finalize_lag(kind, rows[p], count)
        elif kind == 'plv':
            res[p] = finalize_pair('plv', rows[p], count)
        else:
            four = np.stack([rows[p].real, rows[p].imag, chan[ia[p]], chan[ib[p]]], axis=-1)
            res[p] = finalize_pair(kind, four, count)
    return out


def finalize_conn_time(kind: str, sums, power, ia, ib, nsamples: int):
    """The connectivity measure ``kind`` (any name of CONN_OUTS or LAG_OUTS) per epoch, pair and
    scale from the over-time sums of Plan.execute_conn_time over T = ``nsamples`` window samples:
    ``sums`` complex128 (E, P, F) = S (plv, plv_sum, ciplv, ppc: Phi) or float64 (E, P, F, 4) = the lag
    sums, ``power`` float64 (E, C, F) (cross-sum kinds only).  Per pair finalize_pair is applied to
    stack(Re S, Im S, P[:, ia[p]], P[:, ib[p]]), or finalize_lag to the pair's sums, with T in the
    place of the epoch count: csd = S / T, plv = |Phi| / T, pli = |L3| / T and so on (the coherence of
    a channel with itself is exactly 1).  ``cross_sum`` returns (sums, power), ``plv_sum`` and
    ``lag_sum`` return sums; the others (E, P, F): csd and coherency complex128, the rest float64.
    pli2_unbiased and ppc need T >= 2 (ValueError)."""
    if kind not in CONN_OUTS and kind not in LAG_OUTS:
        raise ValueError(f"out must be one of {', '.join({**CONN_OUTS, **LAG_OUTS})}; got {kind!r}")
    if kind == 'cross_sum':
        return sums, power
    if kind in ('plv_sum', 'lag_sum'):
        return sums
    T = int(nsamples)
    if kind in ('pli2_unbiased', 'ppc') and T < 2:
        raise ValueError(f'{kind} needs at least 2 samples in the window, got {T}')
    return _finalize_pairs(kind, sums, power, ia, ib, T, 1)


def check_pac_indices(indices, nchan: int):
    """The pair list of the phase-amplitude calls: ``indices`` = (ip, ia), the phase and the amplitude
    channel of each pair, checked as check_indices checks its lists; None: every channel with itself."""
    if indices is None:
        own = np.arange(int(nchan), dtype=np.int32)
        return own, own.copy()
    return check_indices(indices, nchan)


def check_scales(name: str, positions, nfreq: int) -> np.ndarray:
    """``positions``, a non-empty 1-D list of integer positions in [0, nfreq) into a plan's scale list
    (any list: repeats, any order), as a contiguous int32 array; ValueError naming ``name`` otherwise."""
    try:
        pos = np.asarray(positions)
    except (TypeError, ValueError):
        raise ValueError(f'{name} must be a list of scale positions, got {positions!r}') from None
    if pos.ndim != 1 or pos.size == 0:
        raise ValueError(f'{name} must be a non-empty 1-D list of scale positions, got shape {pos.shape}')
    if not np.issubdtype(pos.dtype, np.integer):
        raise ValueError(f'{name} must hold integer scale positions, got {pos.dtype}')
    if pos.min() < 0 or pos.max() >= nfreq:
        raise ValueError(f'{name} positions must lie in [0, {nfreq}): got {int(pos.min())} .. {int(pos.max())}')
    return np.ascontiguousarray(pos, dtype=np.int32)


def finalize_pac(kind: str, M, amp, phase, ip, ia, nsamples: int):
    """The phase-amplitude coupling measure ``kind`` per epoch, pair and (phase scale, amplitude scale)
    from the sums of Plan.execute_pac over T = ``nsamples`` window samples: ``M`` complex128
    (E, P, Fp, Fa) = sum A u, ``amp`` float64 (E, C, Fa, 2) = {sum A, sum A^2} and ``phase`` complex128
    (E, C, Fp) = sum u, with A the amplitude of channel ia[p] and u the unit phasor of channel ip[p]:
      mvl           |M| / T                              (Canolty et al. 2006)
      mvl_norm      |M| / sum A
      direct_pac    |M| / sqrt(T sum A^2)                (Ozkurt & Schnitzler 2011)
      debiased_pac  |M - (sum u)(sum A) / T| / T         (van Driel et al. 2015)
    float64 (E, P, Fp, Fa); a zero denominator gives 0, not NaN (the wpli convention).  ``pac_sum``
    returns (M, amp, phase) unchanged.  The finalised kinds need T >= 1 (ValueError)."""
    if kind not in PAC_OUTS:
        raise ValueError(f"out must be one of {', '.join(sorted(PAC_OUTS))}; got {kind!r}")
    if kind == 'pac_sum':
        return M, amp, phase
    T = int(nsamples)
    if T < 1:
        raise ValueError(f'{kind} needs at least 1 sample in the window, got {T}')
    M = np.asarray(M, dtype=np.complex128)
    if M.ndim != 4:
        raise ValueError(f'M must be (epochs, pairs, phase scales, amplitude scales), got shape {M.shape}')
    ip, ia = np.asarray(ip, dtype=np.intp), np.asarray(ia, dtype=np.intp)
    if kind == 'mvl':
        return np.abs(M) / T
    amp = np.asarray(amp, dtype=np.float64)
    if kind == 'debiased_pac':
        phase = np.asarray(phase, dtype=np.complex128)
        return np.abs(M - phase[:, ip][:, :, :, None] * amp[:, ia][:, :, None, :, 0] / T) / T
    den = amp[:, ia][:, :, None, :, 0] if kind == 'mvl_norm' else np.sqrt(T * amp[:, ia][:, :, None, :, 1])
    den = np.broadcast_to(den, M.shape)
    zero = den == 0
    return np.where(zero, 0., np.abs(M) / np.where(zero, 1., den))


def check_lags(lags, nsamples: int) -> np.ndarray:
    """``lags`` of the surrogate calls, circular shifts in window samples, as a contiguous int64 array: a 1-D
    list (it may be empty or repeat) of at most NW_PAC_MAX_LAGS integers in [0, T), T = ``nsamples``;
    ValueError naming ``lags`` otherwise."""
    try:
        arr = np.asarray(lags)
    except (TypeError, ValueError):
        raise ValueError(f'lags must be a list of integer shifts, got {lags!r}') from None
    if arr.ndim != 1 or arr.dtype == object:
        raise ValueError(f'lags must be a 1-D list of integer shifts, got shape {arr.shape}')
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f'lags must hold integers, got {arr.dtype}')
    if arr.size > L.NW_PAC_MAX_LAGS:
        raise ValueError(f'lags holds {arr.size} shifts, more than NW_PAC_MAX_LAGS = {L.NW_PAC_MAX_LAGS}')
    if arr.size and (arr.min() < 0 or arr.max() >= nsamples):
        raise ValueError(f'lags must lie in [0, {int(nsamples)}), the window\'s samples: got {int(arr.min())} .. '
                         f'{int(arr.max())}')
    return np.ascontiguousarray(arr, dtype=np.int64)


def draw_lags(nsamples: int, n_surrogates: int = 200, min_lag=None, seed=None) -> np.ndarray:
    """The default lags of the surrogate calls: default_rng(seed).integers(min_lag, T - min_lag + 1,
    n_surrogates) with T = ``nsamples``, so that every cut leaves both blocks at least ``min_lag`` samples long
    (None: max(1, T // 10)); int64.  ValueError unless 1 <= n_surrogates <= NW_PAC_MAX_LAGS, min_lag >= 1 and
    T >= 2 min_lag."""
    import operator
    T = int(nsamples)
    try:
        S = operator.index(n_surrogates)
        lo = max(1, T // 10) if min_lag is None else operator.index(min_lag)
    except TypeError:
        raise ValueError(f'n_surrogates and min_lag must be integers, got {n_surrogates!r} and {min_lag!r}') from None
    if not 1 <= S <= L.NW_PAC_MAX_LAGS:
        raise ValueError(f'n_surrogates must lie in [1, {L.NW_PAC_MAX_LAGS}], got {S}')
    if lo < 1:
        raise ValueError(f'min_lag must be >= 1, got {lo}')
    if T < 2 * lo:
        raise ValueError(f'a window of {T} samples has no lag with both blocks at least min_lag = {lo} long')
    return np.random.default_rng(seed).integers(lo, T - lo + 1, S).astype(np.int64)


def finalize_pac_surr(kind: str, stat_kind: str, M, amp, phase, stat, all, ip, ia, nsamples: int, nlags: int):
    """The surrogate statistic ``stat_kind`` of the coupling measure ``kind`` (mvl, mvl_norm, direct_pac,
    debiased_pac: finalize_pac's) per epoch, pair and (phase scale, amplitude scale) from the sums of
    Plan.execute_pac_surr over T = ``nsamples`` window samples and S = ``nlags`` lags: ``M``, ``amp``, ``phase`` as
    in finalize_pac, ``stat`` float64 (E, P, Fp, Fa, 4) = {sum_s h_s, sum_s q_s, #{s : q_s >= q_0}, max_s q_s} and
    ``all`` complex128 (E, P, Fp, Fa, S) = the surrogate sums M_s (``surrogates`` only; None otherwise), h = |Mc|,
    q = |Mc|^2, Mc = M for the first three kinds and M - (sum u)(sum A) / T for debiased_pac -- the sums must
    come from a call with that centring.  The measure is h times ``norm`` = 1 / (finalize_pac's denominator of
    ``kind``), 0 where that is 0; a circular shift does not change it, so with h_0 = |Mc_0|, mean = sum h / S and
    sd = sqrt(max(0, sum q / S - mean^2)) (the population sd):
      zscore      (h_0 - mean) / sd, 0 where sd = 0       pvalue      (1 + count) / (1 + S)
      surr_mean   mean norm                               surr_std    sd norm
      surr_max    sqrt(max q) norm                        surrogates  |Mc_s| norm, (E, P, Fp, Fa, S)
    float64 (E, P, Fp, Fa).  ``surr_sum`` returns (M, amp, phase, stat, all) unchanged.  The finalised kinds need
    T >= 1 and S >= 1, zscore and surr_std S >= 2 (ValueError)."""
    if kind not in PAC_OUTS or (kind == 'pac_sum' and stat_kind != 'surr_sum'):
        raise ValueError(f"out must be one of {', '.join(sorted(PAC_OUTS - {'pac_sum'}))}; got {kind!r}")
    if stat_kind not in PAC_SURR_STATS:
        raise ValueError(f"stat must be one of {', '.join(sorted(PAC_SURR_STATS))}; got {stat_kind!r}")
    if stat_kind == 'surr_sum':
        return M, amp, phase, stat, all
    T, S = int(nsamples), int(nlags)
    if T < 1:
        raise ValueError(f'{stat_kind} needs at least 1 sample in the window, got {T}')
    need = 2 if stat_kind in ('zscore', 'surr_std') else 1
    if S < need:
        raise ValueError(f'{stat_kind} needs at least {need} surrogate{"s" if need > 1 else ""}, got {S}')
    M = np.asarray(M, dtype=np.complex128)
    if M.ndim != 4:
        raise ValueError(f'M must be (epochs, pairs, phase scales, amplitude scales), got shape {M.shape}')
    ip, ia = np.asarray(ip, dtype=np.intp), np.asarray(ia, dtype=np.intp)
    amp = np.asarray(amp, dtype=np.float64)
    sA = amp[:, ia][:, :, None, :, 0]
    if kind in ('mvl', 'debiased_pac'):
        den = np.full(M.shape, float(T))
    else:
        den = np.broadcast_to(sA if kind == 'mvl_norm' else np.sqrt(T * amp[:, ia][:, :, None, :, 1]), M.shape)
    zero = den == 0
    norm = np.where(zero, 0., 1. / np.where(zero, 1., den))
    D = 0.
    if kind == 'debiased_pac':                    # the device's D: each operation rounded on its own
        P = np.asarray(phase, dtype=np.complex128)[:, ip][:, :, :, None]
        D = (P.real * sA) / T + 1j * ((P.imag * sA) / T)
    if stat_kind == 'surrogates':
        if all is None:
            raise ValueError('surrogates needs the surrogate sums: execute_pac_surr(..., keep_all=True)')
        return np.abs(np.asarray(all, dtype=np.complex128) - np.asarray(D)[..., None]) * norm[..., None]
    stat = np.asarray(stat, dtype=np.float64)
    if stat.shape != M.shape + (4,):
        raise ValueError(f'stat must be {M.shape + (4,)}, got {stat.shape}')
    if stat_kind == 'pvalue':
        return (1. + stat[..., 2]) / (1. + S)
    if stat_kind == 'surr_max':
        return np.sqrt(stat[..., 3]) * norm
    mean = stat[..., 0] / S
    if stat_kind == 'surr_mean':
        return mean * norm
    sd = np.sqrt(np.maximum(0., stat[..., 1] / S - mean * mean))
    if stat_kind == 'surr_std':
        return sd * norm
    Mc = M - D
    h0 = np.sqrt(Mc.real * Mc.real + Mc.imag * Mc.imag)
    flat = sd == 0
    return np.where(flat, 0., (h0 - mean) / np.where(flat, 1., sd))


check_nbins = L.check_nbins     # nbins of the phase-binned calls, checked before any device work


def finalize_pac_bins(kind: str, S, count, ip):
    """The phase-binned coupling measure ``kind`` per epoch, pair and (phase scale, amplitude scale) from
    the sums of Plan.execute_pac_bins: ``S`` float64 (E, P, Fp, Fa, nbins), the amplitude of the pair's
    amplitude channel summed within each phase bin of its phase channel ip[p], and ``count`` float64
    (E, C, Fp, nbins), the samples N_b per bin.  With the mean amplitude A_b = S_b / N_b of a bin and the
    distribution P_b = A_b / sum_b A_b:
      bin_amp     A_b                                               (E, P, Fp, Fa, nbins): the histogram
      mi          (log nbins + sum_b P_b log P_b) / log nbins       (Tort et al. 2010; a bin with P_b = 0 adds 0)
      hr          (max P - min P) / max P                           the height ratio
      pref_phase  theta_b + pi / nbins of the first bin with the largest A_b, theta_b = -pi + 2 pi b / nbins
    mi, hr and pref_phase float64 (E, P, Fp, Fa).  A bin without a sample (N_b = 0) makes bin_amp NaN there
    and mi, hr and pref_phase of the cell NaN; sum_b A_b = 0 with no empty bin gives mi = hr = 0 (the
    zero-denominator convention of finalize_pac).  ``bin_sum`` returns (S, count) unchanged."""
    if kind not in PAC_BIN_OUTS:
        raise ValueError(f"out must be one of {', '.join(sorted(PAC_BIN_OUTS))}; got {kind!r}")
    if kind == 'bin_sum':
        return S, count
    S, count = np.asarray(S, dtype=np.float64), np.asarray(count, dtype=np.float64)
    if S.ndim != 5 or count.ndim != 4 or S.shape[-1] != count.shape[-1]:
        raise ValueError(f'S must be (epochs, pairs, phase scales, amplitude scales, bins) and count (epochs, channels, '
                         f'phase scales, bins), got shapes {S.shape} and {count.shape}')
    nbins = S.shape[-1]
    N = count[:, np.asarray(ip, dtype=np.intp)][:, :, :, None, :]                  # (E, P, Fp, 1, nbins)
    empty = np.broadcast_to(N == 0, S.shape)
    A = np.where(empty, np.nan, S / np.where(N == 0, 1., N))
    if kind == 'bin_amp':
        return A
    bad = empty.any(axis=-1) | np.isnan(A).any(axis=-1)                            # an empty bin, a NaN sum
    tot = np.where(bad, 1., A.sum(axis=-1))
    if kind == 'pref_phase':
        first = np.argmax(np.where(bad[..., None], 0., A), axis=-1)
        return np.where(bad, np.nan, -np.pi + 2 * np.pi * first / nbins + np.pi / nbins)
    zero = tot == 0
    P = np.where(bad[..., None], 1., A) / np.where(zero, 1., tot)[..., None]
    if kind == 'hr':
        top = P.max(axis=-1)
        res = np.where(top == 0, 0., (top - P.min(axis=-1)) / np.where(top == 0, 1., top))
    else:
        plogp = np.where(P > 0, P * np.log(np.where(P > 0, P, 1.)), 0.)
        res = np.where(zero, 0., (np.log(nbins) + plogp.sum(axis=-1)) / np.log(nbins))
    return np.where(bad, np.nan, res)


def _pearson(sxy, sx, sy, sxx, syy, T: int):
    """Pearson's r from the sums over T samples: cov = sxy - sx sy / T, var = sxx - sx^2 / T,
    r = cov / sqrt(var_x var_y), and 0 where a variance is <= 0 (mne's std == 0 -> 1); NaN sums stay NaN."""
    cov = sxy - sx * sy / T
    vx, vy = sxx - sx * sx / T, syy - sy * sy / T
    flat = (vx <= 0) | (vy <= 0)
    return np.where(flat, 0., cov / np.sqrt(np.where(flat, 1., vx * vy)))


def finalize_env(kind: str, pair, chan, ia, ib, nsamples: int):
    """The envelope correlation ``kind`` (Hipp et al. 2012; mne-connectivity's envelope_correlation)
    per epoch, pair p = (a, b) = (ia[p], ib[p]) and scale from the sums of Plan.execute_env_time over
    T = ``nsamples`` window samples: ``chan`` float64 (E, C, F, 2) = {sum A, sum A^2} with A = |y|, and
    ``pair`` float64 (E, P, F) = sum A_a A_b (``env_sum``) or (E, P, F, 6) = {sum u, sum u^2, sum u A_b,
    sum v, sum v^2, sum v A_a} (``env_orth_sum``), u = |Im(y_a conj(y_b) / |y_b|)| being a orthogonalised
    against b and v the reverse.  With r the Pearson correlation over the samples,
      aec              r(A_a, A_b)                      from env_sum        (E, P, F)
      aec_directed     [r(u, A_b), r(v, A_a)]           from env_orth_sum   (E, P, F, 2)
      aec_orth         (|r(u, A_b)| + |r(v, A_a)|) / 2  mne's default (orthogonalize='pairwise', absolute=True)
      aec_orth_signed  (r(u, A_b) + r(v, A_a)) / 2      absolute=False
    r = 0 where a variance is <= 0 (mne's std == 0 -> 1; the wpli convention), and the orthogonalised
    kinds are exactly 0 where ia[p] == ib[p], whatever the sums hold (mne's diagonal).  ``env_sum`` and
    ``env_orth_sum`` return (pair, chan) unchanged.  Plain numpy, float64; the finalised kinds need
    T >= 2 (ValueError)."""
    if kind not in ENV_OUTS:
        raise ValueError(f"out must be one of {', '.join(ENV_OUTS)}; got {kind!r}")
    if kind in ENV_KINDS:
        return pair, chan
    T = int(nsamples)
    if T < 2:
        raise ValueError(f'{kind} needs at least 2 samples in the window, got {T}')
    pair, chan = np.asarray(pair, dtype=np.float64), np.asarray(chan, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.intp), np.asarray(ib, dtype=np.intp)
    if chan.ndim != 4 or chan.shape[-1] != 2:
        raise ValueError(f'chan must be (epochs, channels, scales, 2), got shape {chan.shape}')
    want = 3 if kind == 'aec' else 4
    if pair.ndim != want or (want == 4 and pair.shape[-1] != 6) or pair.shape[1] != ia.size or ia.shape != ib.shape:
        raise ValueError(f"the pair sums of {kind} must be (epochs, {ia.size} pairs, scales{', 6' if want == 4 else ''}), "
                         f'got shape {pair.shape}')
    ca, cb = chan[:, ia], chan[:, ib]                   # (E, P, F, 2): the sums of the pairs' channels
    sa, saa, sb, sbb = ca[..., 0], ca[..., 1], cb[..., 0], cb[..., 1]
    if kind == 'aec':
        return _pearson(pair, sa, sb, saa, sbb, T)
    r_ab = _pearson(pair[..., 2], pair[..., 0], sb, pair[..., 1], sbb, T)
    r_ba = _pearson(pair[..., 5], pair[..., 3], sa, pair[..., 4], saa, T)
    own = (ia == ib)[None, :, None]
    r_ab, r_ba = np.where(own, 0., r_ab), np.where(own, 0., r_ba)
    if kind == 'aec_directed':
        return np.stack([r_ab, r_ba], axis=-1)
    if kind == 'aec_orth':
        return (np.abs(r_ab) + np.abs(r_ba)) / 2
    return (r_ab + r_ba) / 2


def finalize_erpac(kind: str, M, amp, phase, ip, ia, nepochs: int):
    """The event-related phase-amplitude coupling ``kind`` per pair, (phase scale, amplitude scale) and window
    sample from the sums of Plan.execute_erpac over E = ``nepochs`` epochs: ``M`` complex128 (P, Fp, Fa, T) =
    sum_e A u, ``amp`` float64 (C, Fa, T, 2) = {sum A, sum A^2} and ``phase`` float64 (C, Fp, 5, T) = the planes
    sum c, sum s, sum c^2, sum s^2, sum c s, with A the amplitude of channel ia[p] and u = c + i s the unit
    phasor of channel ip[p].  With r the Pearson correlation over the epochs (_pearson: 0 where a variance is
    <= 0), r_xc = r(A, c), r_xs = r(A, s) and r_cs = r(c, s):
      circular       rho = sqrt((r_xc^2 + r_xs^2 - 2 r_xc r_xs r_cs) / (1 - r_cs^2)), the circular-linear
                     correlation (Berens 2009, circ_corrcl; tensorpac's EventRelatedPac(method='circular'),
                     Voytek et al. 2013); a radicand below 0 from rounding gives 0, and 1 - r_cs^2 <= 0 gives 0
                     (the zero-denominator convention of finalize_pac); NaN sums stay NaN
      circular_pval  exp(-E rho^2 / 2): the chi-square survival function with 2 degrees of freedom at E rho^2
      mvl, mvl_norm, direct_pac, debiased_pac   finalize_pac's, with the epoch count in the place of the sample
                     count: one value per window sample
    float64 (P, Fp, Fa, T).  ``erpac_sum`` returns (M, amp, phase) unchanged.  The two circular kinds need
    E >= 2, the others E >= 1 (ValueError)."""
    if kind not in ERPAC_OUTS:
        raise ValueError(f"out must be one of {', '.join(sorted(ERPAC_OUTS))}; got {kind!r}")
    if kind == 'erpac_sum':
        return M, amp, phase
    E = int(nepochs)
    need = 2 if kind.startswith('circular') else 1
    if E < need:
        raise ValueError(f'{kind} needs at least {need} epoch{"s" if need > 1 else ""}, got {E}')
    M = np.asarray(M, dtype=np.complex128)
    amp, phase = np.asarray(amp, dtype=np.float64), np.asarray(phase, dtype=np.float64)
    if M.ndim != 4 or amp.ndim != 4 or amp.shape[-1] != 2 or phase.ndim != 4 or phase.shape[2] != 5:
        raise ValueError(f'M must be (pairs, phase scales, amplitude scales, samples), amp (channels, amplitude scales, '
                         f'samples, 2) and phase (channels, phase scales, 5, samples), got shapes {M.shape}, {amp.shape} '
                         f'and {phase.shape}')
    ip, ia = np.asarray(ip, dtype=np.intp), np.asarray(ia, dtype=np.intp)
    if not kind.startswith('circular'):           # finalize_pac with the sample axis in the place of its epoch axis
        u = np.empty(phase.shape[:2] + phase.shape[3:], dtype=np.complex128)
        u.real, u.imag = phase[:, :, 0], phase[:, :, 1]
        res = finalize_pac(kind, np.moveaxis(M, -1, 0), np.moveaxis(amp, 2, 0), np.moveaxis(u, -1, 0), ip, ia, E)
        return np.ascontiguousarray(np.moveaxis(res, 0, -1))
    sa, saa = amp[ia][:, None, :, :, 0], amp[ia][:, None, :, :, 1]              # (P, 1, Fa, T)
    sc, ss, scc, sss, scs = (phase[ip][:, :, None, k] for k in range(5))         # (P, Fp, 1, T)
    r_xc = _pearson(M.real, sa, sc, saa, scc, E)
    r_xs = _pearson(M.imag, sa, ss, saa, sss, E)
    r_cs = _pearson(scs, sc, ss, scc, sss, E)
    den = 1. - r_cs * r_cs
    flat = den <= 0
    rad = (r_xc * r_xc + r_xs * r_xs - 2. * r_xc * r_xs * r_cs) / np.where(flat, 1., den)
    rho = np.sqrt(np.where(flat | (rad < 0), 0., rad))
    return rho if kind == 'circular' else np.exp(-E * rho * rho / 2.)


def time_window(n: int, decim: int, window, on_device: bool):
    """The window of connectivity_time_batch in a plan's output samples: (t0, t1, step, T).  ``window``
    = (t0, t1) in full-rate samples of an n-sample signal (None: (0, n)); the samples summed are the
    decimated samples j * decim in [t0, t1).  On a device-decimated plan (``on_device``, n_out =
    n // decim) that is [ceil(t0 / decim), ceil(t1 / decim)) with step 1; on a full-rate plan
    t0' = ceil(t0 / decim) * decim with step decim.  ValueError unless 0 <= t0 <= t1 <= n, integers."""
    import operator
    if window is None:
        window = (0, n)
    try:
        t0, t1 = window
        t0, t1 = operator.index(t0), operator.index(t1)
    except (TypeError, ValueError):
        raise ValueError(f'window must be a pair (t0, t1) of integers, got {window!r}') from None
    if not 0 <= t0 <= t1 <= n:
        raise ValueError(f'window must satisfy 0 <= t0 <= t1 <= {n}, got ({t0}, {t1})')
    j0, j1 = -(-t0 // decim), -(-t1 // decim)
    if on_device:
        j1 = min(j1, n // decim)
        j0 = min(j0, j1)
        return j0, j1, 1, j1 - j0
    if decim == 1:
        return t0, t1, 1, t1 - t0
    s0 = min(j0 * decim, t1)
    return s0, t1, decim, -(-(t1 - s0) // decim)


class HostPool:
    """Page-locked result arrays, recycled (nw_host_alloc).

    The reference returns a new array per call (base.py:378-407).  A fresh pageable numpy
    array of a large result is faulted in page by page while the copy-out writes it, which
    bounded the host path at a third of the PCIe rate; a page-locked destination is written
    by DMA directly.  A pooled result is an ordinary numpy array owning its buffer: when the
    caller drops it (and every view of it), the buffer returns to the pool for the next
    result of the same size.  At most ``cap`` bytes are page-locked at a time (results the
    caller keeps count too); past that, results are fresh pageable arrays advised onto huge
    pages (nw_host_advise).  ``min_bytes``: smaller results are not worth a page-locked buffer.

    Released buffers are handed back by a weakref finalizer, which may run inside a garbage
    collection triggered anywhere -- including inside this pool's own locked region.  The
    finalizer therefore never takes the lock or calls into the library: it only appends
    (ptr, nbytes) to a deque (thread-safe append), and the pool drains that queue at the top
    of its next take, outside any finalizer."""

    def __init__(self, cap: int, min_bytes: int = 32 << 20, keep_free: int = 2, alloc=None, free=None,
                 advise=None):
        import collections
        import threading
        self.cap, self.min_bytes, self.keep_free = int(cap), int(min_bytes), int(keep_free)
        self._alloc, self._free_fn = alloc or self._nw_alloc, free or self._nw_free
        self._advise = advise if advise is not None else self._nw_advise
        self._lock = threading.Lock()
        self._free: dict = {}            # nbytes -> [ptr]
        self._returned = collections.deque()   # (ptr, nbytes) released by finalizers, not yet filed
        self.held = 0                    # page-locked bytes, in use or free

    @staticmethod
    def _nw_alloc(nbytes):
        p = ctypes.c_void_p()
        L.check(L.lib().nw_host_alloc(int(nbytes), ctypes.byref(p)))
        return p.value

    @staticmethod
    def _nw_free(ptr):
        L.check(L.lib().nw_host_free(ctypes.c_void_p(ptr)))

    @staticmethod
    def _nw_advise(arr):
        lib = L.lib()
        # an older diagnostic library (NINWAVE_LIB, A/B runs) may lack the symbol: no advice then
        if hasattr(lib, 'nw_host_advise'):
            L.check(lib.nw_host_advise(ctypes.c_void_p(arr.ctypes.data), int(arr.nbytes), None))

    def free_bytes(self) -> int:
        self._drain()
        with self._lock:
            return sum(n * len(v) for n, v in self._free.items())

    def trim(self) -> int:
        """Free every idle pooled buffer now and return the bytes released.  Buffers come back
        lazily: a dropped result is filed by the next empty() / free_bytes() / trim(), so up to
        the cap stays page-locked (and counted in ``held``) after the last result is gone until
        one of them runs."""
        self._drain()
        drop = []
        with self._lock:
            for n, lst in self._free.items():
                while lst:
                    drop.append((lst.pop(), n))
                    self.held -= n
        for ptr, _ in drop:
            self._free_fn(ptr)
        return sum(n for _, n in drop)

    def _drain(self):
        """File the buffers finalizers returned: keep up to keep_free per size, free the rest
        (the library calls happen outside the lock)."""
        drop = []
        with self._lock:
            while self._returned:
                ptr, nbytes = self._returned.popleft()
                lst = self._free.get(nbytes)
                if lst is None:
                    lst = self._free[nbytes] = []
                if len(lst) < self.keep_free:
                    lst.append(ptr)
                else:
                    self.held -= nbytes
                    drop.append(ptr)
        for ptr in drop:
            self._free_fn(ptr)

    def _take(self, nbytes):
        self._drain()
        drop = []
        with self._lock:
            lst = self._free.get(nbytes)
            if lst:
                return lst.pop()
            # make room: drop free buffers of other sizes first
            for n in list(self._free):
                while self._free[n] and self.held + nbytes > self.cap:
                    drop.append(self._free[n].pop())
                    self.held -= n
            ok = self.held + nbytes <= self.cap
            if ok:
                self.held += nbytes
        for ptr in drop:
            self._free_fn(ptr)
        if not ok:
            return None
        try:
            return self._alloc(nbytes)
        except Exception:
            with self._lock:
                self.held -= nbytes
            return None

    def _release(self, ptr, nbytes):
        # finalizer context: no lock, no library call (see the class docstring)
        self._returned.append((ptr, nbytes))

    def empty(self, shape, dtype) -> np.ndarray:
        """np.empty(shape, dtype), page-locked when large enough and within the cap."""
        import weakref
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        if nbytes < self.min_bytes:
            return np.empty(shape, dtype=dt)
        ptr = self._take(nbytes)
        if ptr is None:
            arr = np.empty(shape, dtype=dt)
            self._advise(arr)                # our own fresh array: huge pages for the copy-out
            return arr
        owner = _PooledBuffer(ptr, tuple(int(s) for s in shape), dt)
        f = weakref.finalize(owner, self._release, ptr, nbytes)
        f.atexit = False                 # the process is ending: the OS reclaims it
        return np.asarray(owner)


class _PooledBuffer:
    """Owner of one pooled buffer: exposes it to numpy (__array_interface__); every array or
    view made from it keeps it alive."""

    def __init__(self, ptr, shape, dtype):
        self.__array_interface__ = {'data': (ptr, False), 'shape': shape, 'typestr': dtype.str, 'version': 3}


def host_pinned_array(a) -> bool:
    """Whether numpy array ``a`` (or the array it views) is a pooled page-locked result."""
    b = a
    while b is not None:
        if isinstance(b, _PooledBuffer):
            return True
        b = getattr(b, 'base', None)
    return False


def default_pool_cap(total_ram: int | None = None, local_ranks: int | None = None) -> int:
    """Page-locked bytes one process may pool by default: 8 GiB, at most 1/8 of the host's RAM,
    shared by the ranks of one node (LOCAL_WORLD_SIZE processes each hold their own pool, so
    eight ranks of a node pin no more than one process would).  NINWAVE_HOST_POOL_BYTES
    overrides it."""
    if total_ram is None:
        try:
            total_ram = os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES')
        except (ValueError, OSError, AttributeError):
            total_ram = 64 << 30
    if local_ranks is None:
        local_ranks = local_rank_count()
    return int(min(8 << 30, total_ram // 8) // max(1, local_ranks))


def local_rank_count(env=None) -> int:
    """Processes of this job on this node: torchrun's LOCAL_WORLD_SIZE, else the launcher's
    node-local count (Slurm, Open MPI, MPICH/Hydra), else 1.  Never the global WORLD_SIZE: on a
    multi-node launch that would shrink every rank's pool by the total rank count."""
    env = os.environ if env is None else env
    for k in ('LOCAL_WORLD_SIZE', 'SLURM_NTASKS_PER_NODE', 'OMPI_COMM_WORLD_LOCAL_SIZE', 'MPI_LOCALNRANKS'):
        v = env.get(k)
        if v:
            try:
                return max(1, int(str(v).split('(')[0].split(',')[0]))
            except ValueError:
                continue
    return 1


HOST_POOL = HostPool(int(os.environ.get('NINWAVE_HOST_POOL_BYTES') or default_pool_cap()))


def _ptr(a):
    """The address of a device tensor or a numpy array as a ctypes argument (None: a null pointer)."""
    if a is None:
        return None
    return ctypes.c_void_p(a.data_ptr()) if _is_device_tensor(a) else a.ctypes.data_as(ctypes.c_void_p)


def _epochs(x):
    """(E, C) of an (epochs, channels, n) input."""
    if getattr(x, 'ndim', 0) != 3:
        raise ValueError(f'x must be (epochs, channels, n), got shape {tuple(getattr(x, "shape", ()))}')
    return int(x.shape[0]), int(x.shape[1])


def _conn_kind(out_kind):
    """(kind, lag, single) of a connectivity out_kind; single: one output and no power sums."""
    if out_kind not in CONN_KINDS and out_kind not in LAG_KINDS:
        raise ValueError(f"out_kind must be one of {', '.join({**CONN_KINDS, **LAG_KINDS})}; got {out_kind!r}")
    return {**CONN_KINDS, **LAG_KINDS}[out_kind], out_kind == 'lag_sum', out_kind in ('plv_sum', 'lag_sum')


def _unpack(out, n, what):
    """``out`` as a list of n buffers (None: none given); ValueError(what) for anything else."""
    if out is None:
        return [None] * n
    try:
        outs = list(out)
        if len(outs) != n:
            raise TypeError
    except TypeError:
        raise ValueError(what) from None
    return outs


def _is_device_tensor(a) -> bool:
    return hasattr(a, 'data_ptr') and getattr(a, 'is_cuda', False)


class Plan:
    """One nw_plan: signals of length ``n``, ``nfreq`` scales, compute ``dtype``.  ``decim`` > 1
    (nw_plan_set_decim; where L.decim_supported) keeps every decim-th output sample: the rows
    are ``n_out`` = n // decim long."""

    def __init__(self, n: int, nfreq: int, dtype='float32', device: int = 0, max_batch: int = 1,
                 interpolate: bool = False, engine: str | None = None, timing: bool = False,
                 dedup: bool = True, timing_chain: bool = False, decim: int = 1):
        self.n, self.nfreq, self.device, self.max_batch = int(n), int(nfreq), int(device), int(max_batch)
        self.dtype = np_dtype(dtype)
        self.decim = check_decim(decim)
        self.n_out = self.n
        self.interpolate = bool(interpolate)
        flags = L.NW_INTERPOLATE if interpolate else 0
        if engine == 'rocfft':
            flags |= L.NW_ENGINE_ROCFFT
        elif engine == 'fused':
            flags |= L.NW_ENGINE_FUSED
        elif engine not in (None, 'auto'):
            raise ValueError(f'engine must be rocfft, fused or auto, got {engine!r}')
        if timing:
            flags |= L.NW_TIMING
            if timing_chain:     # a dedicated stream: stage events chained across executes
                flags |= L.NW_TIMING_CHAIN
        if not dedup:            # compute every scale row even when wavelet rows repeat
            flags |= L.NW_NO_DEDUP
        self._h = ctypes.c_void_p()
        L.check(L.lib().nw_plan_create(ctypes.byref(self._h), self.device, self.n, self.max_batch,
                                       self.nfreq, L.NW_F32 if self.dtype == np.float32 else L.NW_F64,
                                       flags))
        self.wavelet_token = None
        if self.decim > 1:
            try:
                L.check(L.lib().nw_plan_set_decim(self._h, self.decim))
            except Exception:
                self.close()
                raise
            self.n_out = self.n // self.decim

    # -- wavelet -----------------------------------------------------------------
    def set_wavelet(self, kind: str, params, freqs, grid: L.nw_grid, table=None, token=None,
                    row_len=None):
        freqs = np.ascontiguousarray(freqs, dtype=np.float64)
        if freqs.shape != (self.nfreq,):
            raise ValueError(f'expected {self.nfreq} freqs, got {freqs.shape}')
        p = np.ascontiguousarray(params if params is not None else [], dtype=np.float64)
        tab_ptr = rl_ptr = None
        if KINDS[kind] == L.NW_TABLE:
            table = np.ascontiguousarray(table, dtype=np.complex128)
            if table.shape != (self.nfreq, grid.len_full):
                raise ValueError(f'table must be ({self.nfreq}, {grid.len_full}), got {table.shape}')
            tab_ptr = table.ctypes.data_as(ctypes.c_void_p)
            if row_len is not None:
                row_len = np.ascontiguousarray(row_len, dtype=np.int64)
                rl_ptr = row_len.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        L.check(L.lib().nw_plan_set_wavelet(
            self._h, KINDS[kind], p.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(p.size),
            freqs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(grid), tab_ptr, rl_ptr))
        self.kind, self.grid = kind, grid
        if kind in TABLE_KINDS:                      # the width the device settled on
            lf = ctypes.c_int64()
            lens = np.empty(self.nfreq, dtype=np.int64)
            L.check(L.lib().nw_plan_wavelet_shape(self._h, ctypes.byref(lf),
                                                  lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            self.grid = L.nw_grid(1.0, lf.value, lf.value)
            self.row_len = lens
        self.wavelet_token = token

    def rows(self) -> np.ndarray:
        """Device-evaluated cached wavelet rows (nfreq, len_full)."""
        dt = self.dtype if self.kind not in TABLE_KINDS else out_dtype(self.dtype, 'cwt')
        out = np.empty((self.nfreq, self.grid.len_full), dtype=dt)
        L.check(L.lib().nw_plan_wavelet_rows(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def row_support(self, scan: bool = False) -> np.ndarray:
        """Two-pass engine diagnostic: each row's last bin above the tail threshold (the row
        pass's pruning bound, nw_plan_row_support); scan=True by scanning every bin."""
        out = np.empty(self.nfreq, dtype=np.int32)
        L.check(L.lib().nw_plan_row_support(self._h, 1 if scan else 0, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- execute -----------------------------------------------------------------
    def execute(self, x, out=None, out_kind: str = 'cwt'):
        """x: (S, n) numpy array (host) -> returns (S, nfreq, n_out); or device tensors."""
        kind = OUT_KINDS[out_kind]
        reduce = out_kind in REDUCTIONS
        if _is_device_tensor(x):
            if out is None:
                raise ValueError('device execute needs an output tensor')
            nsig = self._check_device_input(x)
            self._check_device_buffers(x, out, nsig, out_kind)
            with self._ordered_with_torch(x.device):
                L.check(L.lib().nw_execute(self._h, ctypes.c_void_p(x.data_ptr()), nsig,
                                           ctypes.c_void_p(out.data_ptr()), kind, L.NW_MEM_DEVICE))
            return out
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.shape[-1] != self.n:
            raise ValueError(f'signal length {x.shape[-1]} != plan n {self.n}')
        lead = x.shape[:-1]
        nsig = int(np.prod(lead)) if lead else 1
        odt = out_dtype(self.dtype, out_kind)
        shape = (self.nfreq, self.n_out) if reduce else lead + (self.nfreq, self.n_out)
        if out is None:
            out = HOST_POOL.empty(shape, odt)
        elif out.dtype != odt or not out.flags.c_contiguous or out.size != int(np.prod(shape)):
            raise ValueError('out must be a C-contiguous array of the right dtype and size')
        L.check(L.lib().nw_execute(self._h, x.ctypes.data_as(ctypes.c_void_p), nsig,
                                   out.ctypes.data_as(ctypes.c_void_p), kind, L.NW_MEM_HOST))
        return out

    def execute_pair(self, xa, xb, out=None, out_kind: str = 'cross_sum'):
        """Cross-channel reduction over the signal pairs (xa[e], xb[e]) (nw_execute_pair): xa,
        xb of equal shape (E, n), numpy arrays (host, synchronous) or device tensors
        (asynchronous on the plan stream; ``out`` required).  ``cross_sum`` -> float64
        (nfreq, n_out, 4) = {Re S_ab, Im S_ab, P_aa, P_bb}; ``plv_sum`` -> complex128
        (nfreq, n_out); see finalize_pair.  ``lag_sum`` -> float64 (nfreq, n_out, 4) = the
        phase-lag sums {L0, L1, L2, L3}; see finalize_lag.  The plan needs max_batch >= 2."""
        kind = _conn_kind(out_kind)[0]
        dev = _is_device_tensor(xa) or _is_device_tensor(xb)
        if dev:
            if out is None:
                raise ValueError('device execute needs an output tensor')
            npairs = self._check_device_input(xa)
            if self._check_device_input(xb) != npairs:
                raise ValueError('the two inputs must hold the same number of signals')
        else:
            xa = np.ascontiguousarray(xa, dtype=self.dtype)
            xb = np.ascontiguousarray(xb, dtype=self.dtype)
            if xa.shape != xb.shape:
                raise ValueError(f'the two inputs must have the same shape, got {xa.shape} and {xb.shape}')
            if xa.ndim < 1 or xa.shape[-1] != self.n:
                raise ValueError(f'signal length {xa.shape[-1] if xa.ndim else None} != plan n {self.n}')
            npairs = int(np.prod(xa.shape[:-1])) if xa.ndim > 1 else 1
        plv = out_kind == 'plv_sum'
        spec = ('sums', (self.nfreq, self.n_out) + (() if plv else (4,)), np.complex128 if plv else np.float64, False)
        outs = self._outputs(xa, [out], [spec], ndarray_only=False)
        self._epoch_execute(L.lib().nw_execute_pair, xa, (_ptr(xb), npairs), outs, (kind,))
        return outs[0]

    def execute_conn(self, x, indices=None, out=None, out_kind: str = 'cross_sum'):
        """Multi-channel connectivity sums (nw_execute_conn): x (E, C, n), the E epochs of C
        channels, every signal transformed once and reduced on the device into the sums of the
        pairs ``indices`` = (ia, ib) (default all_pairs(C)).  ``cross_sum`` -> (cross complex128
        (P, nfreq, n_out) = sum_e y_a conj(y_b), power float64 (C, nfreq, n_out) = sum_e |y_c|^2);
        ``plv_sum`` -> complex128 (P, nfreq, n_out); see finalize_conn.  numpy arrays: synchronous,
        ``out`` optional.  Device tensors: asynchronous on the plan stream, ``out`` required:
        (cross, power) tensors for cross_sum (power may be None: not formed), the tensor for
        plv_sum.  ``lag_sum`` -> float64 (P, nfreq, n_out, 4), the phase-lag sums of every pair (see
        finalize_lag), one array or tensor as plv_sum.  The plan needs max_batch >= C (a chunk holds
        max_batch // C epochs)."""
        kind, lag, single = _conn_kind(out_kind)
        nep, nchan = _epochs(x)
        ia, ib = check_indices(indices, nchan)
        npairs = int(ia.size)
        x = self._epoch_input(x, nep * nchan, out)
        specs = [('cross', (npairs, self.nfreq, self.n_out) + ((4,) if lag else ()),
                  np.float64 if lag else np.complex128, False),
                 ('power', (nchan, self.nfreq, self.n_out), np.float64, True)][:1 if single else 2]
        cross, power = (out, None) if single or out is None else out
        # (this call and execute_pair never asked that host outputs be ndarrays)
        outs = self._outputs(x, [cross, power], specs, ndarray_only=False)
        self._epoch_execute(L.lib().nw_execute_conn, x, (nep, nchan, _ptr(ia), _ptr(ib), npairs), outs, (kind,))
        return out if _is_device_tensor(x) else outs[0] if single else (outs[0], outs[1])

    def execute_conn_time(self, x, indices=None, window=None, step: int = 1, out=None, out_kind: str = 'cross_sum'):
        """Over-time connectivity sums (nw_execute_conn_time): x (E, C, n) as in execute_conn, every
        signal transformed once and reduced on the device along the samples t0, t0 + step, ... < t1
        of ``window`` = (t0, t1), in the plan's OUTPUT samples (None: (0, n_out)), into one value per
        epoch, pair of ``indices`` and scale.  ``cross_sum`` -> (sums complex128 (E, P, nfreq), power
        float64 (E, C, nfreq)); ``plv_sum`` -> complex128 (E, P, nfreq); ``lag_sum`` -> float64
        (E, P, nfreq, 4); see finalize_conn_time.  numpy arrays: synchronous, ``out`` optional.  Device
        tensors: asynchronous on the plan stream, ``out`` required ((sums, power) for cross_sum, power
        may be None: not formed).  The plan needs max_batch >= C."""
        kind, lag, single = _conn_kind(out_kind)
        nep, nchan = _epochs(x)
        ia, ib = check_indices(indices, nchan)
        npairs = int(ia.size)
        t0, t1, step = self._window(window, step)
        x = self._epoch_input(x, nep * nchan, out)
        specs = [('sums', (nep, npairs, self.nfreq) + ((4,) if lag else ()),
                  np.float64 if lag else np.complex128, False),
                 ('power', (nep, nchan, self.nfreq), np.float64, True)][:1 if single else 2]
        sums, power = (out, None) if single or out is None else out
        outs = self._outputs(x, [sums, power], specs)
        self._epoch_execute(L.lib().nw_execute_conn_time, x, (nep, nchan, _ptr(ia), _ptr(ib), npairs, t0, t1, step),
                            outs, (kind,))
        return out if _is_device_tensor(x) else outs[0] if single else (outs[0], outs[1])

    def execute_env_time(self, x, indices=None, window=None, step: int = 1, out=None, out_kind: str = 'env_orth_sum'):
        """Envelope-correlation sums (nw_execute_env_time): x (E, C, n), ``indices``, ``window`` (the
        plan's OUTPUT samples; None: (0, n_out)) and ``step`` as in execute_conn_time, every signal
        transformed once and reduced on the device.  Returns (pair, chan): ``env_sum`` -> pair float64
        (E, P, nfreq) = sum A_a A_b, ``env_orth_sum`` -> pair float64 (E, P, nfreq, 6) = {sum u, sum u^2,
        sum u A_b, sum v, sum v^2, sum v A_a}; chan float64 (E, C, nfreq, 2) = {sum A, sum A^2}; see
        finalize_env.  numpy arrays: synchronous, ``out`` optional.  Device tensors: asynchronous on the
        plan stream, ``out`` = (pair, chan) required (chan may be None: not formed).  The plan needs
        max_batch >= C."""
        if out_kind not in ENV_KINDS:
            raise ValueError(f"out_kind must be one of {', '.join(ENV_KINDS)}; got {out_kind!r}")
        kind = ENV_KINDS[out_kind]
        nep, nchan = _epochs(x)
        ia, ib = check_indices(indices, nchan)
        npairs = int(ia.size)
        t0, t1, step = self._window(window, step)
        x = self._epoch_input(x, nep * nchan, out)
        dev = _is_device_tensor(x)
        outs = _unpack(out, 2, 'device output must be (pair, chan) tensors (chan may be None)' if dev else
                       'out must be (pair, chan) arrays')
        outs = self._outputs(x, outs, [('pair', (nep, npairs, self.nfreq) + ((6,) if kind == L.NW_ENV_ORTH else ()),
                                        np.float64, False), ('chan', (nep, nchan, self.nfreq, 2), np.float64, True)])
        self._epoch_execute(L.lib().nw_execute_env_time, x, (nep, nchan, _ptr(ia), _ptr(ib), npairs, t0, t1, step),
                            outs, (kind,))
        return out if dev else tuple(outs)

    def execute_pac(self, x, indices=None, phase=None, amp=None, window=None, step: int = 1, out=None):
        """Phase-amplitude coupling sums (nw_execute_pac): x (E, C, n) as in execute_conn_time, every
        signal transformed once and reduced on the device along the samples t0, t0 + step, ... < t1 of
        ``window`` (the plan's OUTPUT samples; None: (0, n_out)).  ``indices`` = (ip, ia): the phase and
        the amplitude channel of each pair (None: every channel with itself); ``phase`` / ``amp``:
        positions into the plan's scale list (any lists: repeats, a scale in both).  Returns (M
        complex128 (E, P, Fp, Fa) = sum |y_a| u_p, amp float64 (E, C, Fa, 2) = {sum |y|, sum |y|^2}, phase
        complex128 (E, C, Fp) = sum u); see finalize_pac.  numpy arrays: synchronous, ``out`` optional.
        Device tensors: asynchronous on the plan stream, ``out`` = (M, amp, phase) required (amp and
        phase may be None: not formed).  The plan needs max_batch >= C."""
        nep, nchan = _epochs(x)
        ip, ia = check_pac_indices(indices, nchan)
        npairs = int(ip.size)
        fph, fam = check_scales('phase', phase, self.nfreq), check_scales('amp', amp, self.nfreq)
        nph, nam = int(fph.size), int(fam.size)
        t0, t1, step = self._window(window, step)
        x = self._epoch_input(x, nep * nchan, out)
        dev = _is_device_tensor(x)
        outs = _unpack(out, 3, 'device output must be (M, amp, phase) tensors (amp and phase may be None)' if dev else
                       'out must be (M, amp, phase) arrays')
        outs = self._outputs(x, outs, [('M', (nep, npairs, nph, nam), np.complex128, False),
                                       ('amp', (nep, nchan, nam, 2), np.float64, True),
                                       ('phase', (nep, nchan, nph), np.complex128, True)])
        self._epoch_execute(L.lib().nw_execute_pac, x,
                            (nep, nchan, _ptr(ip), _ptr(ia), npairs, _ptr(fph), nph, _ptr(fam), nam, t0, t1, step), outs)
        return out if dev else tuple(outs)

    def execute_pac_surr(self, x, lags, indices=None, phase=None, amp=None, window=None, step: int = 1,
                         centre: str = 'plain', keep_all: bool = False, out=None):
        """Time-lag surrogate sums of the coupling (nw_execute_pac_surr): x, ``indices``, ``phase``, ``amp``,
        ``window`` and ``step`` as in execute_pac; ``lags``: circular shifts of the amplitude inside the window,
        integers in [0, T) (check_lags; any list, at most NW_PAC_MAX_LAGS); ``centre``: 'plain' (mvl, mvl_norm,
        direct_pac) or 'debiased' (debiased_pac: M - (sum u)(sum A) / T).  Returns (M, amp, phase) as execute_pac,
        bit for bit, then stat float64 (E, P, Fp, Fa, 4) = {sum_s |Mc_s|, sum_s |Mc_s|^2, #{s : |Mc_s|^2 >=
        |Mc_0|^2}, max_s |Mc_s|^2} and, with ``keep_all``, all complex128 (E, P, Fp, Fa, S) = M_{lags[s]}; see
        finalize_pac_surr.  numpy arrays: synchronous, ``out`` optional.  Device tensors: asynchronous on the
        plan stream, ``out`` = (M, amp, phase, stat[, all]) required (amp and phase may be None: not returned).
        The plan needs max_batch >= C; one chunk's listed rows are staged in fp64 on the device
        ((max_batch // C) C (2 Fp + Fa) T values)."""
        nep, nchan = _epochs(x)
        ip, ia = check_pac_indices(indices, nchan)
        npairs = int(ip.size)
        fph, fam = check_scales('phase', phase, self.nfreq), check_scales('amp', amp, self.nfreq)
        nph, nam = int(fph.size), int(fam.size)
        t0, t1, step = self._window(window, step)
        lags = check_lags(lags, len(range(t0, t1, step)))
        nlags = int(lags.size)
        if centre not in PAC_SURR_CENTRES:
            raise ValueError(f"centre must be one of {', '.join(PAC_SURR_CENTRES)}; got {centre!r}")
        x = self._epoch_input(x, nep * nchan, out)
        dev = _is_device_tensor(x)
        nout = 5 if keep_all else 4
        outs = _unpack(out, nout, 'device output must be (M, amp, phase, stat[, all]) tensors (amp and phase may be None)'
                       if dev else 'out must be (M, amp, phase, stat[, all]) arrays')
        specs = [('M', (nep, npairs, nph, nam), np.complex128, False), ('amp', (nep, nchan, nam, 2), np.float64, True),
                 ('phase', (nep, nchan, nph), np.complex128, True), ('stat', (nep, npairs, nph, nam, 4), np.float64, False),
                 ('all', (nep, npairs, nph, nam, nlags), np.complex128, False)][:nout]
        outs = self._outputs(x, outs, specs)
        self._epoch_execute(L.lib().nw_execute_pac_surr, x,
                            (nep, nchan, _ptr(ip), _ptr(ia), npairs, _ptr(fph), nph, _ptr(fam), nam, t0, t1, step,
                             _ptr(lags), nlags, PAC_SURR_CENTRES[centre]), outs + [None] * (5 - nout))
        return out if dev else tuple(outs)

    def execute_erpac(self, x, indices=None, phase=None, amp=None, window=None, step: int = 1, out=None):
        """Event-related phase-amplitude coupling sums (nw_execute_erpac): x, ``indices``, ``phase``, ``amp``,
        ``window`` and ``step`` as in execute_pac, the sums taken over the EPOCHS at each of the window's T samples
        t0, t0 + step, ... < t1.  Returns (M complex128 (P, Fp, Fa, T) = sum_e |y_a| u_p, amp float64
        (C, Fa, T, 2) = {sum_e |y|, sum_e |y|^2}, phase float64 (C, Fp, 5, T) = the planes sum_e c, s, c^2, s^2, c s
        of the unit phasor u = c + i s); see finalize_erpac.  Every value is added in epoch order in one fp64
        accumulator: it does not depend on the lists, the window or the chunks.  numpy arrays: synchronous,
        ``out`` optional.  Device tensors: asynchronous on the plan stream, ``out`` = (M, amp, phase) required (amp
        and phase may be None: not formed).  The plan needs max_batch >= C; the accumulators are read and written
        once per chunk of max_batch // C epochs, so the rate depends on the epochs per chunk."""
        nep, nchan = _epochs(x)
        ip, ia = check_pac_indices(indices, nchan)
        npairs = int(ip.size)
        fph, fam = check_scales('phase', phase, self.nfreq), check_scales('amp', amp, self.nfreq)
        nph, nam = int(fph.size), int(fam.size)
        t0, t1, step = self._window(window, step)
        count = len(range(t0, t1, step))
        x = self._epoch_input(x, nep * nchan, out)
        dev = _is_device_tensor(x)
        outs = _unpack(out, 3, 'device output must be (M, amp, phase) tensors (amp and phase may be None)' if dev else
                       'out must be (M, amp, phase) arrays')
        outs = self._outputs(x, outs, [('M', (npairs, nph, nam, count), np.complex128, False),
                                       ('amp', (nchan, nam, count, 2), np.float64, True),
                                       ('phase', (nchan, nph, 5, count), np.float64, True)])
        self._epoch_execute(L.lib().nw_execute_erpac, x,
                            (nep, nchan, _ptr(ip), _ptr(ia), npairs, _ptr(fph), nph, _ptr(fam), nam, t0, t1, step), outs)
        return out if dev else tuple(outs)

    def execute_pac_bins(self, x, indices=None, phase=None, amp=None, window=None, step: int = 1, nbins: int = 18,
                         out=None):
        """Phase-binned phase-amplitude coupling sums (nw_execute_pac_bins): x, ``indices``, ``phase``,
        ``amp``, ``window`` and ``step`` as in execute_pac; ``nbins`` even, 2 .. 36.  Returns (S float64
        (E, P, Fp, Fa, nbins) = the amplitude |y_a| summed within each phase bin of y_p, count float64
        (E, C, Fp, nbins) = the samples per bin); bin b holds the phases [-pi + 2 pi b / nbins, -pi + 2 pi
        (b + 1) / nbins), by the rule of ninwave.h on the table L.pac_bin_edges(nbins); see finalize_pac_bins.
        numpy arrays: synchronous, ``out`` optional.  Device tensors: asynchronous on the plan stream,
        ``out`` = (S, count) required (count may be None: not formed).  The plan needs max_batch >= C."""
        nep, nchan = _epochs(x)
        ip, ia = check_pac_indices(indices, nchan)
        npairs = int(ip.size)
        fph, fam = check_scales('phase', phase, self.nfreq), check_scales('amp', amp, self.nfreq)
        nph, nam = int(fph.size), int(fam.size)
        nbins = check_nbins(nbins)
        t0, t1, step = self._window(window, step)
        x = self._epoch_input(x, nep * nchan, out)
        dev = _is_device_tensor(x)
        outs = _unpack(out, 2, 'device output must be (S, count) tensors (count may be None)' if dev else
                       'out must be (S, count) arrays')
        outs = self._outputs(x, outs, [('S', (nep, npairs, nph, nam, nbins), np.float64, False),
                                       ('count', (nep, nchan, nph, nbins), np.float64, True)])
        self._epoch_execute(L.lib().nw_execute_pac_bins, x,
                            (nep, nchan, _ptr(ip), _ptr(ia), npairs, _ptr(fph), nph, _ptr(fam), nam, t0, t1, step, nbins),
                            outs)
        return out if dev else tuple(outs)

    def _window(self, window, step):
        """(t0, t1, step) of an over-time call, checked: ``window`` in the plan's output samples."""
        import operator
        try:
            t0, t1 = (0, self.n_out) if window is None else window
            t0, t1, step = operator.index(t0), operator.index(t1), operator.index(step)
        except (TypeError, ValueError):
            raise ValueError(f'window must be a pair (t0, t1) of integers and step an integer, got {window!r} and '
                             f'{step!r}') from None
        if step < 1:
            raise ValueError(f'step must be >= 1, got {step}')
        if not 0 <= t0 <= t1 <= self.n_out:
            raise ValueError(f'window must satisfy 0 <= t0 <= t1 <= n_out = {self.n_out}, got ({t0}, {t1})')
        return t0, t1, step

    def _epoch_input(self, x, nsig, out):
        """The (E, C, n) input of an epoch-chunk call, checked: a device tensor (``out`` is then
        required), or a host array made contiguous in the plan's dtype."""
        if _is_device_tensor(x):
            if out is None:
                raise ValueError('device execute needs output tensors')
            if self._check_device_input(x) != nsig:
                raise ValueError(f'signal length {x.shape[-1]} != plan n {self.n}')
            return x
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.shape[-1] != self.n:
            raise ValueError(f'signal length {x.shape[-1]} != plan n {self.n}')
        return x

    def _outputs(self, x, outs, specs, ndarray_only=True):
        """The output buffers of an epoch-chunk call on x's side: those of ``specs`` (name, shape, numpy
        dtype, optional), then None for the rest of ``outs`` (outputs this call does not form).  Device:
        every tensor validated; an optional one may be None (not formed).  Host: a missing array is
        allocated, a given one validated."""
        outs = list(outs)
        for k, (name, shape, dt, optional) in enumerate(specs):
            t, count = outs[k], int(np.prod(shape))
            if not _is_device_tensor(x):
                if t is None:
                    t = outs[k] = np.empty(shape, dtype=dt)
                if ((ndarray_only and not isinstance(t, np.ndarray)) or t.dtype != dt or not t.flags.c_contiguous
                        or t.size != count):
                    raise ValueError('out must be C-contiguous arrays of the right dtype and size')
            elif t is not None or not optional:
                import torch
                tdt = torch.complex128 if dt is np.complex128 else torch.float64
                if not _is_device_tensor(t) or t.dtype != tdt:
                    raise ValueError(f'device output {name} must be a {tdt} tensor on device {self.device}')
                if not t.is_contiguous() or t.numel() != count:
                    raise ValueError(f'device output {name} must be contiguous and hold {count} values')
                if t.device.index != self.device:
                    raise ValueError(f'device buffers must live on device {self.device}')
        return outs

    def _epoch_execute(self, fn, x, head, outs, tail=()):
        """fn(plan, x, *head, *outs, *tail, mem) on x's side; device tensors in order with torch's stream."""
        dev = _is_device_tensor(x)
        with self._ordered_with_torch(x.device) if dev else contextlib.nullcontext():
            L.check(fn(self._h, _ptr(x), *head, *map(_ptr, outs), *tail, L.NW_MEM_DEVICE if dev else L.NW_MEM_HOST))

    def stream_ptr(self) -> int:
        """The hipStream_t the plan launches on."""
        h = ctypes.c_void_p()
        L.check(L.lib().nw_plan_get_stream(self._h, ctypes.byref(h)))
        return h.value or 0

    @contextlib.contextmanager
    def _ordered_with_torch(self, device):
        """Order a device-tensor execute with torch's current stream on both sides: the
        plan stream waits for the work that produced the input, and torch's stream waits
        for the plan's kernels before anything later reads the output or the caching
        allocator reuses either buffer."""
        import torch
        cur = torch.cuda.current_stream(device)
        plan_stream = torch.cuda.ExternalStream(self.stream_ptr(), device=device)
        plan_stream.wait_stream(cur)
        try:
            yield
        finally:
            cur.wait_stream(plan_stream)

    def execute_ptr(self, x_ptr: int, nsig: int, out_ptr: int, out_kind: str = 'cwt'):
        """Raw device pointers on the plan's device (asynchronous on the plan stream; the
        caller orders it against its own streams, e.g. with plan.sync()).  The output holds
        (nsig, nfreq, n_out) values, (nfreq, n_out) for the reductions."""
        L.check(L.lib().nw_execute(self._h, ctypes.c_void_p(x_ptr), int(nsig), ctypes.c_void_p(out_ptr),
                                   OUT_KINDS[out_kind], L.NW_MEM_DEVICE))

    def _check_device_input(self, x) -> int:
        """The input half of _check_device_buffers: a contiguous (nsig, n) tensor of the
        compute dtype on the plan's device, whole rows only.  Returns nsig."""
        import torch
        want_x = torch.float32 if self.dtype == np.float32 else torch.float64
        if not _is_device_tensor(x):
            raise ValueError(f'device input must be a torch tensor on device {self.device}')
        if x.dtype != want_x:
            raise ValueError(f'device input must be {want_x}, got {x.dtype}')
        if not x.is_contiguous():
            raise ValueError('device input must be contiguous')
        if x.numel() % self.n:
            raise ValueError(f'device input of {x.numel()} values is not a whole number of '
                             f'{self.n}-sample signals')
        if x.device.index != self.device:
            raise ValueError(f'device input must live on device {self.device}, got {x.device}')
        return x.numel() // self.n

    def _check_device_buffers(self, x, out, nsig, out_kind):
        import torch
        if self._check_device_input(x) != nsig:
            raise ValueError('device buffer sizes do not match (S, n) -> (S, nfreq, n_out) / (nfreq, n_out)')
        want_o = {('cwt', np.float32): torch.complex64, ('cwt', np.float64): torch.complex128}.get(
            (out_kind, self.dtype.type), x.dtype)
        if out_kind == 'power_sum':
            want_o = torch.float64
        elif out_kind == 'phase_sum':
            want_o = torch.complex128
        if out.dtype != want_o:
            raise ValueError(f'device buffers must be {x.dtype} in / {want_o} out')
        if not out.is_contiguous():
            raise ValueError('device buffers must be contiguous')
        rows = 1 if out_kind in REDUCTIONS else nsig
        if out.numel() != rows * self.nfreq * self.n_out:
            raise ValueError('device buffer sizes do not match (S, n) -> (S, nfreq, n_out) / (nfreq, n_out)')
        if out.device.index != self.device:
            raise ValueError(f'device buffers must live on device {self.device}')

    # -- misc --------------------------------------------------------------------
    def set_stream(self, stream_ptr: int | None):
        L.check(L.lib().nw_plan_set_stream(self._h, ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def sync(self):
        L.check(L.lib().nw_plan_sync(self._h))

    def stats(self) -> dict:
        s = L.nw_stats()
        L.check(L.lib().nw_plan_stats(self._h, ctypes.byref(s)))
        d = s.as_dict()
        d['engine'] = 'fused' if d['engine'] == L.NW_ENGINE_FUSED else 'rocfft'
        return d

    def reset_stats(self):
        L.check(L.lib().nw_plan_reset_stats(self._h))

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            L.lib().nw_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def execute_multi(plans, x: np.ndarray, out_kind: str = 'cwt', shard: str = 'signals') -> np.ndarray:
    """Several single-device plans, one host thread each.
    shard='signals': identical plans, contiguous blocks of the host signals per device
    (nw_execute_multi).  shard='scales': plan i holds the i-th contiguous slice of the
    scale list and transforms every signal for it (nw_execute_multi_scales) -- the split
    for one long signal (C5)."""
    if shard not in ('signals', 'scales'):
        raise ValueError(f"shard must be 'signals' or 'scales', got {shard!r}")
    p0 = plans[0]
    x = np.ascontiguousarray(x, dtype=p0.dtype)
    lead = x.shape[:-1]
    nsig = int(np.prod(lead)) if lead else 1
    nf = sum(p.nfreq for p in plans) if shard == 'scales' else p0.nfreq
    if any(p.n_out != p0.n_out for p in plans):
        raise ValueError('plans must share decim')
    shape = (nf, p0.n_out) if out_kind in REDUCTIONS else lead + (nf, p0.n_out)
    out = HOST_POOL.empty(shape, out_dtype(p0.dtype, out_kind))
    arr = (ctypes.c_void_p * len(plans))(*[p.handle.value for p in plans])
    fn = L.lib().nw_execute_multi_scales if shard == 'scales' else L.lib().nw_execute_multi
    L.check(fn(arr, len(plans), x.ctypes.data_as(ctypes.c_void_p), nsig,
               out.ctypes.data_as(ctypes.c_void_p), OUT_KINDS[out_kind]))
    return out


def execute_multi_device(plans, xs, outs, out_kind: str = 'cwt'):
    """Device-resident sharding (nw_execute_multi_device): plan i transforms
    the torch tensor xs[i] (on plan i's device, (nsig_i, n)) into outs[i]; for the
    reductions outs[0] receives the (F, n) result over every signal of every device.
    One host thread per device; returns when every device is done."""
    if not (len(plans) == len(xs) == len(outs)):
        raise ValueError('one input and one output tensor per plan')
    red = out_kind in REDUCTIONS
    nsig = []
    for i, (p, x, o) in enumerate(zip(plans, xs, outs)):
        # every input is validated (dtype, contiguity, whole rows, device): its raw pointer
        # goes to nw_execute as device memory of plan i; for the reductions only outs[0] is
        # written, so the other outputs may be None
        ns = p._check_device_input(x)
        if not red or i == 0:
            p._check_device_buffers(x, o, ns, out_kind)
        nsig.append(ns)
    import torch
    for p, x in zip(plans, xs):                 # inputs produced on torch's streams are complete
        torch.cuda.current_stream(x.device).synchronize()
    P = ctypes.c_void_p
    arr = (P * len(plans))(*[p.handle.value for p in plans])
    xa = (P * len(plans))(*[x.data_ptr() for x in xs])
    oa = (P * len(plans))(*[(o.data_ptr() if o is not None else 0) for o in outs])
    na = (ctypes.c_int64 * len(plans))(*nsig)
    L.check(L.lib().nw_execute_multi_device(arr, len(plans), xa, na, oa, OUT_KINDS[out_kind]))
    return outs[0] if red else outs


def make_wavelets(kind: str, params, freqs, sfreq: float, real_wave_length: float, device: int = 0) -> list:
    """Time-domain wavelets of a stock kind on the device (nw_make_wavelets,
    base.py:346-376): a list of complex128 rows of their true (ragged) lengths."""
    fr = np.ascontiguousarray(list(freqs), dtype=np.float64)
    p = np.ascontiguousarray(params if params is not None else [], dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int64)
    lens = np.zeros(fr.size, dtype=np.int64)
    mx = ctypes.c_int64()
    args = (device, KINDS[kind], p.ctypes.data_as(dp), int(p.size), fr.ctypes.data_as(dp), int(fr.size),
            float(sfreq), float(real_wave_length))
    L.check(L.lib().nw_make_wavelets(*args, None, ctypes.byref(mx), lens.ctypes.data_as(ip)))
    out = np.zeros((fr.size, mx.value), dtype=np.complex128)
    L.check(L.lib().nw_make_wavelets(*args, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(mx),
                                     lens.ctypes.data_as(ip)))
    return [out[i, :lens[i]].copy() for i in range(fr.size)]
