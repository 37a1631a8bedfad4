"""EpochsWavelet: CWT over the epochs of one channel (reference mneutils.py:9-71).

The reference maps ``wavelet.cwt`` over epochs in a Python loop (mneutils.py:39);
here all epochs go to the device in one batched call (``cwt_batch``) with the
same cache semantics: the wavelet table is built from the first epoch's length
unless the wavelet already holds one (``reuse=True``)."""
from __future__ import annotations

import numpy as np

from .base import WaveletBase


class EpochsWavelet:
    """Wavelet transform of mne-style epochs (anything with ``info['sfreq']``,
    ``ch_names`` and ``get_data() -> (epochs, channels, samples)``)."""

    def __init__(self, epochs, wavelet: WaveletBase) -> None:
        self.epochs = epochs
        self.wavelet = wavelet
        wavelet.sfreq = self.epochs.info['sfreq']           # mneutils.py:24

    def _waves(self, ch_name: str) -> np.ndarray:
        idx = self.epochs.ch_names.index(ch_name)
        return self.epochs.get_data()[:, idx, :]

    def _pick(self, ch_names) -> np.ndarray:
        """The (E, C, N) data of the channels ``ch_names``, in that order."""
        idx = [self.epochs.ch_names.index(c) for c in list(ch_names)]
        return self.epochs.get_data()[:, idx, :]

    def _padded(self, n: int, padding: float):
        """(k, n - k), k = round(padding * sfreq): the window of n-sample epochs that ``padding`` seconds
        on each side leave; ValueError if it is empty."""
        if not padding >= 0:
            raise ValueError(f'padding must be >= 0 seconds, got {padding!r}')
        k = int(round(padding * self.epochs.info['sfreq']))
        if k >= n - k:
            raise ValueError(f'padding of {padding} s ({k} samples on each side) leaves no sample of the {n}')
        return k, n - k

    def cwt(self, ch_name: str, freqs, decim: int = 1) -> np.ndarray:
        """(epochs, F, N) complex (mneutils.py:26-40); ``decim`` (MNE's, as MorseMNE.cwt passes
        it, wavelets.py:170-191) keeps every decim-th sample of the last axis, here and below."""
        return self.wavelet.cwt_batch(self._waves(ch_name), freqs, reuse=True, decim=decim)

    def power(self, ch_name: str, freqs, decim: int = 1) -> np.ndarray:
        """Epoch-mean of |cwt|^2, (F, N) (mneutils.py:42-55), reduced on the device:
        the (epochs, F, N) CWT is never materialised (fp64 sums in epoch order)."""
        return self.wavelet.cwt_batch(self._waves(ch_name), freqs, reuse=True, out='power_mean', decim=decim)

    def itc(self, ch_name: str, freqs, decim: int = 1) -> np.ndarray:
        """Inter-trial coherence |mean(cwt/|cwt|)|, (F, N) (mneutils.py:57-71), reduced
        on the device; a point where some epoch has |cwt| = 0 is NaN, as in the reference."""
        return self.wavelet.cwt_batch(self._waves(ch_name), freqs, reuse=True, out='itc', decim=decim)

    # -- connectivity between two channels: cross-channel epoch reductions on the device
    #    (WaveletBase.cross_batch; no reference counterpart) --------------------------------
    def _cross(self, ch_a: str, ch_b: str, freqs, out: str, decim: int) -> np.ndarray:
        return self.wavelet.cross_batch(self._waves(ch_a), self._waves(ch_b), freqs, reuse=True, out=out,
                                        decim=decim)

    def csd(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Epoch-mean cross-spectrum mean_e cwt_a conj(cwt_b), (F, N) complex128."""
        return self._cross(ch_a, ch_b, freqs, 'csd', decim)

    def coherence(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """|S_ab| / sqrt(P_aa P_bb) of the epoch sums, (F, N) float64."""
        return self._cross(ch_a, ch_b, freqs, 'coherence', decim)

    def imcoh(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Imaginary part of the coherency S_ab / sqrt(P_aa P_bb), (F, N) float64."""
        return self._cross(ch_a, ch_b, freqs, 'imcoh', decim)

    def plv(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Phase-locking value |mean_e (cwt_a / |cwt_a|) conj(cwt_b / |cwt_b|)|, (F, N) float64; a
        point where some epoch has |cwt| = 0 is NaN, as itc."""
        return self._cross(ch_a, ch_b, freqs, 'plv', decim)

    # -- phase-lag connectivity between two channels (WaveletBase.lag_batch): measures that do not
    #    respond to zero-lag coupling, mne-connectivity's names ----------------------------------
    def _lag(self, ch_a: str, ch_b: str, freqs, out: str, decim: int) -> np.ndarray:
        return self.wavelet.lag_batch(self._waves(ch_a), self._waves(ch_b), freqs, reuse=True, out=out, decim=decim)

    def pli(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Phase-lag index |mean_e sgn Im(cwt_a conj(cwt_b))|, (F, N) float64."""
        return self._lag(ch_a, ch_b, freqs, 'pli', decim)

    def dpli(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Directed phase-lag index: the mean Heaviside step of Im(cwt_a conj(cwt_b)) (H(0) = 1/2),
        (F, N) float64."""
        return self._lag(ch_a, ch_b, freqs, 'dpli', decim)

    def wpli(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Weighted phase-lag index |sum_e m_e| / sum_e |m_e| with m_e = Im(cwt_a conj(cwt_b)), (F, N)
        float64; 0 where every m_e is 0."""
        return self._lag(ch_a, ch_b, freqs, 'wpli', decim)

    def wpli2_debiased(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Debiased squared wPLI ((sum m)^2 - sum m^2) / ((sum |m|)^2 - sum m^2), (F, N) float64."""
        return self._lag(ch_a, ch_b, freqs, 'wpli2_debiased', decim)

    def ciplv(self, ch_a: str, ch_b: str, freqs, decim: int = 1) -> np.ndarray:
        """Corrected imaginary PLV |Im plv| / sqrt(1 - (Re plv)^2) of the mean unit-phasor product,
        (F, N) float64; NaN where some |cwt| = 0, as plv."""
        return self._lag(ch_a, ch_b, freqs, 'ciplv', decim)

    def lag_connectivity(self, ch_names, freqs, method: str = 'wpli', indices=None, decim: int = 1):
        """``method`` (lag_batch's outs: pli, pli2_unbiased, dpli, wpli, wpli2_debiased, ciplv, ppc,
        lag_sum) for the channel pairs ``indices`` of ``ch_names``, (P, F, N), as connectivity."""
        waves = self._pick(ch_names)
        return self.wavelet.lag_connectivity_batch(waves, freqs, reuse=True, out=method, indices=indices, decim=decim)

    # -- over-time connectivity: one value per epoch, pair and scale, the sums taken over the samples
    #    of each epoch on the device (WaveletBase.connectivity_time_batch) -------------------------
    def connectivity_time(self, ch_names, freqs, method: str = 'coherence', indices=None, padding: float = 0.,
                          decim: int = 1, average: bool = False):
        """``method`` (connectivity's and lag_connectivity's) per epoch, (E, P, F): what
        mne-connectivity's spectral_connectivity_time returns.  ``padding`` in seconds, as there: with
        k = round(padding * sfreq) the samples [k, N - k) of every epoch are summed (ValueError if
        that window is empty).  ``average=True``: the mean over the epochs, (P, F)."""
        waves = self._pick(ch_names)
        window = self._padded(waves.shape[-1], padding)
        return self.wavelet.connectivity_time_batch(waves, freqs, reuse=True, out=method, indices=indices,
                                                    window=window, decim=decim, average=average)

    # -- envelope correlation: the amplitude-coupling counterpart, per epoch, pair and scale
    #    (WaveletBase.envelope_correlation_batch) ------------------------------------------------
    def envelope_correlation(self, ch_names, freqs, method: str = 'aec_orth', indices=None, padding: float = 0.,
                             decim: int = 1, average: bool = False):
        """``method`` (envelope_correlation_batch's outs: aec_orth, aec_orth_signed, aec_directed, aec,
        env_sum, env_orth_sum) per epoch, (E, P, F): what mne-connectivity's envelope_correlation
        returns per pair, with the wavelet rows as the analytic signals.  ``indices`` = (ia, ib),
        positions in ``ch_names`` (default: every pair a < b); ``padding`` as in connectivity_time;
        ``average=True``: the mean over the epochs, (P, F)."""
        waves = self._pick(ch_names)
        window = self._padded(waves.shape[-1], padding)
        return self.wavelet.envelope_correlation_batch(waves, freqs, reuse=True, out=method, indices=indices,
                                                       window=window, decim=decim, average=average)

    # -- phase-amplitude coupling: one comodulogram per epoch and pair (WaveletBase.pac_batch) ------
    def pac(self, ch_names, phase_freqs, amp_freqs, method: str = 'direct_pac', indices=None, padding: float = 0.,
            decim: int = 1, average: bool = False):
        """``method`` (pac_batch's outs: mvl, mvl_norm, direct_pac, debiased_pac, pac_sum) between the
        phase at ``phase_freqs`` and the amplitude at ``amp_freqs``, (E, P, Fp, Fa): the concatenated
        frequency list is transformed once.  ``indices`` = (phase channels, amplitude channels),
        positions in ``ch_names`` (default: every channel with itself); ``padding`` as in
        connectivity_time; ``average=True``: the mean over the epochs, (P, Fp, Fa)."""
        waves = self._pick(ch_names)
        window = self._padded(waves.shape[-1], padding)
        pf, af = list(phase_freqs), list(amp_freqs)
        return self.wavelet.pac_batch(waves, pf + af, reuse=False, phase=np.arange(len(pf)),
                                      amp=np.arange(len(pf), len(pf) + len(af)), out=method, indices=indices,
                                      window=window, decim=decim, average=average)

    def pac_surrogates(self, ch_names, phase_freqs, amp_freqs, method: str = 'direct_pac', stat: str = 'zscore',
                       n_surrogates: int = 200, lags=None, min_lag=None, seed=None, indices=None, padding: float = 0.,
                       decim: int = 1, average: bool = False):
        """``stat`` (pac_surrogates_batch's: zscore, pvalue, surr_mean, surr_std, surr_max, surrogates, surr_sum)
        of the coupling ``method`` (mvl, mvl_norm, direct_pac, debiased_pac) against time-lag surrogates, the
        amplitude shifted circularly inside the kept samples: (E, P, Fp, Fa), and (E, P, Fp, Fa, S) for
        ``surrogates``.  ``n_surrogates``, ``lags`` (in the kept, decimated samples), ``min_lag`` and ``seed`` as in
        pac_surrogates_batch; frequency lists, ``indices``, ``padding``, ``decim`` and ``average`` as in pac
        (``average=True``: zscore, surr_mean and surr_std only)."""
        waves = self._pick(ch_names)
        window = self._padded(waves.shape[-1], padding)
        pf, af = list(phase_freqs), list(amp_freqs)
        return self.wavelet.pac_surrogates_batch(waves, pf + af, reuse=False, phase=np.arange(len(pf)),
                                                 amp=np.arange(len(pf), len(pf) + len(af)), out=method, stat=stat,
                                                 n_surrogates=n_surrogates, lags=lags, min_lag=min_lag, seed=seed,
                                                 indices=indices, window=window, decim=decim, average=average)

    # -- event-related phase-amplitude coupling: across the epochs, one time course per pair and cell
    #    (WaveletBase.erpac_batch) ---------------------------------------------------------------
    def erpac(self, ch_names, phase_freqs, amp_freqs, method: str = 'circular', indices=None, padding: float = 0.,
              decim: int = 1):
        """``method`` (erpac_batch's outs: circular, circular_pval, mvl, mvl_norm, direct_pac, debiased_pac,
        erpac_sum) between the phase at ``phase_freqs`` and the amplitude at ``amp_freqs`` ACROSS the epochs
        at every sample, (P, Fp, Fa, N'): when, relative to the event, the coupling appears (tensorpac's
        EventRelatedPac).  Frequency lists, ``indices``, ``padding`` and ``decim`` as in pac: the samples
        [k, N - k), k = round(padding * sfreq), are kept."""
        waves = self._pick(ch_names)
        window = self._padded(waves.shape[-1], padding)
        pf, af = list(phase_freqs), list(amp_freqs)
        return self.wavelet.erpac_batch(waves, pf + af, reuse=False, phase=np.arange(len(pf)),
                                        amp=np.arange(len(pf), len(pf) + len(af)), out=method, indices=indices,
                                        window=window, decim=decim)

    def pac_bins(self, ch_names, phase_freqs, amp_freqs, method: str = 'mi', nbins: int = 18, indices=None,
                 padding: float = 0., decim: int = 1, average: bool = False):
        """``method`` (pac_bins_batch's outs: mi, hr, pref_phase, bin_amp, bin_sum) from the amplitude at
        ``amp_freqs`` averaged within ``nbins`` bins of the phase at ``phase_freqs``: (E, P, Fp, Fa), and
        (E, P, Fp, Fa, nbins) for the histogram ``bin_amp``.  Frequency lists, ``indices``, ``padding``, ``decim``
        and ``average`` as in pac (``average=True`` is a ValueError for pref_phase and bin_sum)."""
        waves = self._pick(ch_names)
        window = self._padded(waves.shape[-1], padding)
        pf, af = list(phase_freqs), list(amp_freqs)
        return self.wavelet.pac_bins_batch(waves, pf + af, reuse=False, phase=np.arange(len(pf)),
                                           amp=np.arange(len(pf), len(pf) + len(af)), out=method, nbins=nbins,
                                           indices=indices, window=window, decim=decim, average=average)

    # -- connectivity between many channels: one transform per epoch and channel, every pair's
    #    sums from it (WaveletBase.connectivity_batch; no reference counterpart) ---------------
    def connectivity(self, ch_names, freqs, method: str = 'coherence', indices=None, decim: int = 1):
        """``method`` (cross_batch's outs: coherence, imcoh, coherency, csd, plv, ...) for the
        channel pairs ``indices`` = (ia, ib), positions in ``ch_names`` (default: every pair
        a < b), (P, F, N): what mne-connectivity's spectral_connectivity_epochs(..., indices=...)
        returns per pair in its cwt_morlet mode."""
        waves = self._pick(ch_names)
        return self.wavelet.connectivity_batch(waves, freqs, reuse=True, out=method, indices=indices, decim=decim)
