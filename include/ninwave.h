/*
 * ninwave.h — C ABI of libninwave.so, the MI355X (gfx950) FFT-domain CWT engine.
 *
 * This is the drop-in boundary for ninwavelets' hot path:
 *   WaveletBase.cwt / power / abs         reference base.py:378-443
 *   WaveletBase.make_fft_wavelet(s)       reference base.py:221-279
 *   WaveletBase._setup_trans_shape        reference base.py:173-194
 *   pad_to / interpolate_alias            reference base.py:75-82, 107-123
 *   Morse / Morlet / Shannon spectra      reference wavelets.py:65-74, 132-136, 256-262
 *   EpochsWavelet.cwt (batched caller)    reference mneutils.py:26-40
 * The reference is pure Python/numpy, so it has no FFI of its own; the Python
 * host layer (ninwavelets_amd/_lib.py, ctypes) binds exactly these symbols, and
 * INTEGRATION.md shows the binding a maintainer would add to the reference.
 *
 * Conventions
 *  - Every function returns int status: NW_OK (0) or a negative NW_E* code;
 *    nw_last_error() returns a thread-local message for the last failure.
 *  - Plain pointers and sizes only.  Host buffers are C-contiguous row-major.
 *  - A plan is bound to one device and one HIP stream; it is not reentrant.
 *  - Complex numbers are interleaved (re, im) of the plan's real dtype.
 */
#ifndef NINWAVE_H
#define NINWAVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define NW_OK              0
#define NW_E_INVALID      -1   /* bad argument (maps to ValueError) */
#define NW_E_HIP          -2   /* HIP runtime error */
#define NW_E_ROCFFT       -3   /* rocFFT error */
#define NW_E_NOMEM        -4   /* device allocation failed */
#define NW_E_STATE        -5   /* call out of order (e.g. execute before set_wavelet) */
#define NW_E_NODEVICE     -6   /* no HIP device visible */
#define NW_E_BOUNDS       -7   /* debug library only: a kernel bounds check failed */

/* compute dtypes (the arithmetic type of the whole path) */
#define NW_F32 0
#define NW_F64 1

/* wavelet kinds */
#define NW_MORSE   1   /* params: b, r                      wavelets.py:38-74  */
#define NW_MORLET  2   /* params: sigma, gabor(0/1)         wavelets.py:110-144 */
#define NW_SHANNON 3   /* params: none (freq is ignored)    wavelets.py:256-262 */
#define NW_TABLE   4   /* complex128 rows supplied by the host (WaveletMode.Normal,
                          user plugins overriding trans_formula/formula)          */
#define NW_MEXICAN_HAT 5  /* params: sigma, sfreq, real_wave_length   wavelets.py:194-228 */
#define NW_HAAR        6  /* params: sfreq, real_wave_length          wavelets.py:265-280
                             Both are WaveletMode.Normal tables built ON THE DEVICE
                             (base.py:249-256): the time-domain wavelet on np.arange's
                             grid, zero-padded to ~sfreq*real_wave_length, fp64 rocFFT,
                             |Re| + i|Im| (+ interpolate_alias), ragged row lengths. */

/* plan flags */
#define NW_INTERPOLATE   0x1u  /* zero the upper half of fft(x) (interpolate_alias, base.py:400-401) */
#define NW_ENGINE_ROCFFT 0x10u /* force: rocFFT fwd -> K1 multiply -> rocFFT inv -> K2 epilogue   */
#define NW_ENGINE_FUSED  0x20u /* force: rocFFT fwd -> fused multiply+LDS inverse FFT+epilogue
                                  (n > 16384: the two-pass form, nw_large.hip; n not a power
                                  of two >= 1024 with 2n-1 <= 16384 fp32 / 8192 fp64: the
                                  chirp-z form, nw_chirp.hip)                                  */
#define NW_TIMING        0x100u/* record HIP events around every stage (nw_plan_stats)            */
#define NW_TIMING_CHAIN  0x800u/* with NW_TIMING: the plan's stream carries nothing but this plan's
                                  executes between two nw_plan_sync / nw_plan_stats calls (a
                                  dedicated benchmark stream), so each stage -- the first of an
                                  execute too -- starts at the previous stage's end event.  No
                                  event marker enters the stream around kernel-only stages (their
                                  stop events ride on the kernel dispatches themselves); rocFFT
                                  and memcpy stages still record their end events.  The first
                                  stage of an execute includes any idle gap since the previous
                                  execute                                                       */
#define NW_NO_CHIRP      0x400u/* auto engine: keep the rocFFT engine for lengths the chirp-z fused
                                  form would take (non-power-of-two n, 2n-1 <= 16384 fp32 /
                                  8192 fp64, and n < 1024; up to n < 16384 / 8192 when every
                                  wavelet row's support K fits n + K - 1 <= 16384 / 8192)      */
#define NW_NO_DEDUP      0x200u/* compute every scale row even when wavelet rows repeat (by
                                  default rows with identical W -- Shannon ignores f
                                  (wavelets.py:256-262), repeated freqs -- are computed once
                                  and copied: bit-identical output, nw_stats.unique_rows)      */

/* execute outputs */
#define NW_OUT_CWT   0   /* complex (S, F, N)   base.py:378-407 */
#define NW_OUT_ABS   1   /* real    (S, F, N)   base.py:427-443 */
#define NW_OUT_POWER 2   /* real    (S, F, N)   base.py:409-425 */
/* Reductions over the nsig signals (EpochsWavelet, mneutils.py:42-71): out is (F, N),
 * summed in signal order in fp64 on the device; (E, F, N) is never materialised.  The sums do
 * not depend on the plan's max_batch (nw_stats.reduce_path: on either path). */
#define NW_OUT_POWER_MEAN 3  /* real (F, N), compute dtype: mean_s |y|^2    mneutils.py:42-55 */
#define NW_OUT_ITC        4  /* real (F, N), compute dtype: |mean_s y/|y||  mneutils.py:57-71;
                                |y| = 0 gives NaN, as 0/0 does in the reference */
#define NW_OUT_POWER_SUM  5  /* float64 (F, N): sum_s |y|^2 (partial sums to combine over
                                devices or ranks, then divide by the total count) */
#define NW_OUT_PHASE_SUM  6  /* complex128 (F, N): sum_s y/|y| (partial sums; ITC = |sum/S|) */
/* Cross-channel reductions over the npairs signal pairs (a_e, b_e) of nw_execute_pair (no
 * reference counterpart: connectivity from the per-epoch CWT), summed in pair order in fp64 on
 * the device; nw_execute and nw_execute_multi* do not take them. */
#define NW_OUT_CROSS_SUM  7  /* float64 (F, N, 4): {Re S_ab, Im S_ab, P_aa, P_bb} per point with
                                S_ab = sum_e y_a,e conj(y_b,e), P_aa = sum_e |y_a,e|^2 */
#define NW_OUT_PLV_SUM    8  /* complex128 (F, N): sum_e (y_a,e/|y_a,e|) conj(y_b,e/|y_b,e|);
                                some |y| = 0 gives NaN there, as NW_OUT_ITC */
#define NW_OUT_LAG_SUM    9  /* float64 (F, N, 4): the phase-lag sums {L0, L1, L2, L3} = sum_e of
                                {m_e, |m_e|, m_e^2, sgn m_e} with m_e = Im y_a,e conj(y_b,e), formed
                                as the imaginary term of NW_OUT_CROSS_SUM (L0 is Im S_ab of the
                                per-signal-rows path bit for bit); sgn(+-0) = 0 and sgn(NaN) = NaN, so
                                L3 is an exact integer and a NaN row makes all four NaN.  What PLI,
                                dPLI, wPLI and their debiased forms need (nw_execute_pair,
                                nw_execute_conn) */

/* memory placement of x / out in nw_execute */
#define NW_MEM_HOST   0
#define NW_MEM_DEVICE 1

/* Analytic-spectrum grid of one cache build (base.py:173-194, 238-246, 274-276):
 *   nu_j = j * delta for j < len_valid, and zero for len_valid <= j < len_full.
 * delta = 1/(n/sfreq); len_full is the row length of the reference's cached
 * wavelet (len(np.arange(...)), doubled by the hstack when interpolating). */
typedef struct nw_grid {
    double  delta;
    int64_t len_full;
    int64_t len_valid;
} nw_grid;

/* Per-stage device time accumulated since the plan was created or reset. */
typedef struct nw_stats {
    int64_t executes;       /* nw_execute calls */
    int64_t chunks;         /* device chunks run */
    double  ms_forward;     /* rocFFT forward (R2C) */
    double  ms_multiply;    /* K1 spectrum multiply (rocFFT engine) */
    double  ms_inverse;     /* rocFFT inverse (rocFFT engine) */
    double  ms_epilogue;    /* K2 |.| / |.|^2 (rocFFT engine) */
    double  ms_fused;       /* fused multiply + inverse FFT + epilogue (fused engine) */
    double  ms_copy;        /* copies (host<->device, input staging, spectrum transposes) */
    int64_t launches_multiply;
    int64_t launches_fused;    /* output-kernel launches of the fused engine (chirp-z form: one per
                                  transform size M that holds rows, per chunk) */
    int64_t engine;         /* NW_ENGINE_ROCFFT or NW_ENGINE_FUSED actually used */
    double  ms_rows;        /* fused engine, n > 16384: pass-1 row FFTs (ms_fused then times
                               pass 2, the column FFTs + epilogue; the spectrum transpose is
                               timed in ms_copy) */
    int64_t launches_rows;
    double  ms_expand;      /* repeated rows: copies of the computed unique rows */
    int64_t launches_expand;
    int64_t unique_rows;    /* scale rows actually computed (nfreq unless rows repeat) */
    int64_t kernel;         /* NW_K_*: the output-writing kernel of the last chunk */
    int64_t device_bytes;   /* device memory the plan holds now: input / spectrum / output /
                               reduction buffers, wavelet tables, two-pass scratch, rocFFT work
                               (it grows as calls need larger buffers; the Python classes
                               bound their plan cache by it) */
    int64_t reduce_path;    /* NW_REDUCE_*: how the last reduction executed formed its sums */
} nw_stats;

/* nw_stats.reduce_path */
#define NW_REDUCE_NONE     0   /* no reduction executed yet                                     */
#define NW_REDUCE_ROWS     1   /* per-signal rows per chunk, added in signal order in fp64     */
#define NW_REDUCE_PARTIALS 2   /* fp64 block partial sums inside the transform kernel          */
#define NW_REDUCE_CONN     3   /* nw_execute_conn: per-signal rows per chunk, every pair's sums
                                  added in epoch order by nw_conn_accumulate_kernel            */
#define NW_REDUCE_CONN_TIME 4  /* nw_execute_conn_time: per-signal rows per chunk, every (epoch,
                                  pair, scale) summed over the window by nw_conn_time_kernel    */
#define NW_REDUCE_PAC      5   /* nw_execute_pac: per-signal rows per chunk, every (epoch, pair,
                                  phase scale, amplitude scale) summed over the window by
                                  nw_pac_kernel                                                 */
#define NW_REDUCE_ENV      6   /* nw_execute_env_time: per-signal rows per chunk, every (epoch,
                                  pair, scale) summed over the window by nw_env_time_kernel    */
#define NW_REDUCE_PAC_BINS 7   /* nw_execute_pac_bins: per-signal rows per chunk, every (epoch, pair,
                                  phase scale, amplitude scale, phase bin) summed over the window
                                  by nw_pac_bins_kernel                                         */
#define NW_REDUCE_ERPAC 8      /* nw_execute_erpac: per-signal rows per chunk, every (pair, phase
                                  scale, amplitude scale, window sample) added in epoch order by
                                  nw_erpac_kernel                                               */
#define NW_REDUCE_PAC_SURR 9   /* nw_execute_pac_surr: per-signal rows per chunk, staged once as unit
                                  phasors and magnitudes, every (epoch, pair, phase scale, amplitude
                                  scale) summed once per lag by nw_pac_surr_kernel              */

/* nw_stats.kernel: which kernel wrote the output rows (the dominant kernel of a step) */
#define NW_K_NONE        0
#define NW_K_FUSED       1   /* nw_fused_kernel (one pass, one signal per lane value)        */
#define NW_K_FUSED_PAIR  2   /* nw_fused_pair_kernel (one pass, two signals per lane value)  */
#define NW_K_CHIRP       3   /* nw_chirp_kernel (chirp-z form)                               */
#define NW_K_TWO_PASS    4   /* rows_kernel + cols_kernel (n > 16384; cols writes the output) */
#define NW_K_MULTIPLY    5   /* k1_multiply + rocFFT inverse (+ k2_epilogue): rocFFT engine   */
#define NW_K_FUSED_DECIM 6   /* nw_fused_decim_kernel (one pass, decimated rows)             */

typedef struct nw_plan nw_plan;

const char* nw_last_error(void);
const char* nw_version(void);
/* Diagnostics on stderr ("[ninwave] ..." lines): 0 silent, 1 plan / engine / reduction-path
 * decisions and every error status, 2 also every launch stage (and its time under NW_TIMING).
 * Default: the NW_LOG environment variable, else 0.  Returns the previous level. */
int nw_set_log_level(int level);
/* 1 in the debug library (libninwave_debug.so: kernel bounds checks, every call synchronous,
 * NW_E_BOUNDS names the failing file:line), 0 in the product library. */
int nw_debug_bounds(void);
/* Debug library: launches one kernel whose checks fail on purpose (no memory is touched) and
 * returns the resulting NW_E_BOUNDS status; the product library returns NW_E_STATE. */
int nw_debug_selftest(int device);
int nw_device_count(int* n);

/* Host-only (no GPU): the grid of the reference's make_fft_wavelet(freq, real_length)
 * -- cwt passes real_length = n / sfreq (base.py:395).  Replaces _setup_trans_shape
 * (base.py:173-194) as called from base.py:238-245. */
int nw_trans_grid(double real_length, double sfreq, int interpolate, nw_grid* grid);

/* Host-only (no GPU): whether the fused engine supports (n, dtype): power-of-two n with
 * 1024 <= n <= 16384 in one on-chip pass, or 2^15 <= n <= 2^24 in its two-pass form (row
 * FFTs of W*X, then column FFTs + epilogue); fp32 and fp64 alike. */
int nw_fused_supported(int64_t n, int dtype);

/* Host-only (no GPU): whether a plan of (n, dtype) can decimate its output rows by decim on
 * the device (nw_plan_set_decim): power-of-two n with 2048 <= n <= 16384, power-of-two
 * decim >= 2 with n / decim >= 1024, fp32 or fp64.  The reference's decim is the one
 * MorseMNE.cwt passes through to MNE (wavelets.py:170-191). */
int nw_decim_supported(int64_t n, int dtype, int decim);

/* Host-only (no GPU): whether nw_execute_pair of a plan of (n, dtype) whose wavelet is of
 * `kind` forms the sums of out_kind (NW_OUT_CROSS_SUM / NW_OUT_PLV_SUM) as block partial sums
 * inside the transform kernel (nw_stats.reduce_path = NW_REDUCE_PARTIALS); elsewhere the
 * per-signal rows of each chunk are reduced (NW_REDUCE_ROWS).  1 for fp32, n = 1024 / 2048 /
 * 4096 and the analytic kinds (NW_MORSE, NW_MORLET, NW_SHANNON); plans with decim > 1 or repeated
 * rows keep the chunk path.  The same terms are added either way (regrouped fp64 additions; the
 * unit phasors of NW_OUT_PLV_SUM by rsqrt instead of hypot and divide, a few fp64 ulp).
 * 0 for NW_OUT_LAG_SUM at every size: its sums always come from the per-signal rows. */
int nw_pair_partials_supported(int64_t n, int dtype, int kind, int out_kind);

/* Create a plan for signals of n samples, up to max_batch signals per device
 * chunk, nfreq scales.  flags: NW_INTERPOLATE | NW_ENGINE_* | NW_TIMING. */
int nw_plan_create(nw_plan** plan, int device, int64_t n, int64_t max_batch,
                   int32_t nfreq, int dtype, uint32_t flags);

/* Attach the wavelet (the reference's cached fft_wavelets, base.py:258-279).
 *   freqs[nfreq]: scale frequencies; grid: the cache-build grid (nw_trans_grid of
 *   the build length -- it may differ from the plan's n: base.py:394-397 reuses
 *   the cache and pad_to's it to the current n).
 *   params: NW_MORSE {b, r}; NW_MORLET {sigma, gabor[, c, k]} (c, k of wavelets.py:118-122,
 *   derived from sigma when absent); NW_SHANNON {}; NW_TABLE {}.
 *   table: NW_TABLE only, complex128 [nfreq][grid.len_full], copied to the device.
 *   row_len: NW_TABLE only, optional [nfreq] true length of each row (rows are
 *   left-aligned in the table); the reference pad_to's every row on its own
 *   (base.py:396-397) and time-domain rows can differ by one sample.  NULL: all
 *   rows are grid.len_full long. */
int nw_plan_set_wavelet(nw_plan* plan, int kind, const double* params, int nparams,
                        const double* freqs, const nw_grid* grid, const void* table,
                        const int64_t* row_len);

/* Time decimation (the decim of MorseMNE.cwt, wavelets.py:170-191): every output row of the
 * plan holds the n / decim samples y[0], y[decim], y[2 decim], ... of the full row, computed as
 * the (n / decim)-point inverse transform of the folded product (exact; nw_fused_decim_kernel),
 * so outputs are (nsig, nfreq, n / decim), or (nfreq, n / decim) for the reduction kinds.  The
 * wavelet is still attached for the full length n.  Call it before the first nw_execute
 * (NW_E_STATE afterwards); decim = 1 is a no-op; NW_E_INVALID where nw_decim_supported is 0 or
 * the plan runs the rocFFT engine.  Plans of one nw_execute_multi* call must share decim. */
int nw_plan_set_decim(nw_plan* plan, int decim);

/* Shape of the attached wavelet's cached rows: len_full (the table width; for the
 * device-built NW_MEXICAN_HAT / NW_HAAR tables the longest row) and, if row_len is not
 * NULL, each row's true length [nfreq] (ragged Normal-mode rows, base.py:253-254). */
int nw_plan_wavelet_shape(nw_plan* plan, int64_t* len_full, int64_t* row_len);

/* Evaluate the attached wavelet rows on the device and copy them to the host:
 * out[nfreq][len_full] of the plan dtype (real for analytic kinds, complex for the
 * table kinds) -- the reference's self.fft_wavelets. */
int nw_plan_wavelet_rows(nw_plan* plan, void* out_host);

/* Diagnostic: the W-row support the two-pass engine (2^15 <= n <= 2^24) prunes its row pass
 * to -- kmax_out[nfreq] = the last bin k whose |W_f[k]| exceeds the tail threshold (2^-72 fp64,
 * 2^-56 fp32, of the row's max |W|; -1 for an all-zero row) of every scale of the plan.  method
 * 0: as the engine builds it (no full scan for Morse / Morlet / Shannon rows), 1: by scanning every bin
 * (the reference the tests compare method 0 with).  No reference counterpart: the reference
 * multiplies every bin (base.py:404-406); the cut bins together move y by < n * 2^-72 (fp64)
 * of the signal's scale.  NW_E_STATE for plans on another engine. */
int nw_plan_row_support(nw_plan* plan, int method, int32_t* kmax_out);

/* Run the CWT of nsig signals x[nsig][n] (plan dtype) into out[nsig][nfreq][n]
 * (complex for NW_OUT_CWT, real otherwise), or (F, N) for the reduction kinds
 * NW_OUT_POWER_MEAN .. NW_OUT_PHASE_SUM.  mem = NW_MEM_HOST: synchronous;
 * NW_MEM_DEVICE: x/out are device pointers on the plan's device, the call is
 * asynchronous on the plan stream (see nw_plan_sync). */
int nw_execute(nw_plan* plan, const void* x, int64_t nsig, void* out, int out_kind, int mem);

/* Cross-channel epoch reductions: the CWT rows y_a,e of xa[e] and y_b,e of xb[e] (both
 * (npairs, n) of the plan dtype) reduced over e = 0 .. npairs-1 into out, NW_OUT_CROSS_SUM
 * (float64 (F, n_out, 4)), NW_OUT_PLV_SUM (complex128 (F, n_out)) or NW_OUT_LAG_SUM (float64
 * (F, n_out, 4), always NW_REDUCE_ROWS); every sum in fp64, in pair
 * order; (npairs, F, N) is never materialised.  The plan stages the inputs interleaved
 * a0, b0, a1, b1, ... into its own buffer, max_batch / 2 pairs per chunk, so max_batch must
 * be >= 2 (NW_E_INVALID).  mem as in nw_execute (host: synchronous; device: asynchronous on
 * the plan stream).  npairs = 0 gives zero sums.  A decimated plan reduces its n / decim rows. */
int nw_execute_pair(nw_plan* plan, const void* xa, const void* xb, int64_t npairs, void* out,
                    int out_kind, int mem);

/* Host-only (no GPU): the pair tiling nw_execute_conn uses.  tile_of_pair[npairs] (may be NULL)
 * receives each pair's tile; *ntiles the count; limits[3] (may be NULL) = {kConnCh, kConnPairs,
 * sample tile}.  NW_E_INVALID: nchan < 1, an index outside [0, nchan), npairs < 0. */
int nw_conn_tiles(int32_t nchan, const int32_t* ia, const int32_t* ib, int64_t npairs,
                  int32_t* tile_of_pair, int64_t* ntiles, int32_t* limits);

/* Multi-channel connectivity: the sums of nw_execute_pair for npairs channel pairs
 * (ia[p], ib[p]) of nchan channels from ONE transform of every epoch and channel.
 * x: (nepochs, nchan, n) of the plan dtype.  ia, ib: HOST arrays [npairs] (any list: repeats,
 * a > b, a == b).
 * NW_OUT_CROSS_SUM: out_cross complex128 (npairs, F, n_out) = sum_e y_a conj(y_b),
 *                   out_power float64 (nchan, F, n_out) = sum_e |y_c|^2 (may be NULL).
 * NW_OUT_PLV_SUM:   out_cross complex128 (npairs, F, n_out) = sum_e unit phasor products;
 *                   out_power must be NULL.
 * NW_OUT_LAG_SUM:   out_cross float64 (npairs, F, n_out, 4) = the phase-lag sums {L0 .. L3};
 *                   out_power must be NULL.
 * Every sum in fp64 in epoch order, the terms those of nw_execute_pair's per-signal-rows path
 * (bit-identical to it for the same two channels, however the epochs are chunked).
 * Chunks of max_batch / nchan epochs: max_batch >= nchan, else NW_E_INVALID.  mem as in
 * nw_execute_pair.  nepochs = 0 or npairs = 0: zero sums.  Decimated plans reduce n / decim rows.
 * The fp64 accumulators live in the plan (nw_stats.device_bytes); NW_E_NOMEM if they do not fit. */
int nw_execute_conn(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                    const int32_t* ia, const int32_t* ib, int64_t npairs,
                    void* out_cross, void* out_power, int out_kind, int mem);

/* Host-only (no GPU): *count = T, the number of samples t0, t0 + step, ... < t1 of a window of
 * nw_execute_conn_time.  NW_E_INVALID unless 0 <= t0 <= t1 <= n_out and step >= 1. */
int nw_conn_time_count(int64_t n_out, int64_t t0, int64_t t1, int64_t step, int64_t* count);

/* Over-time connectivity: nw_execute_conn's sums taken over the SAMPLES of each epoch instead of
 * over the epochs -- one value per epoch, pair and scale (mne-connectivity's
 * spectral_connectivity_time).  x, ia, ib, nchan, chunking (max_batch / nchan epochs,
 * max_batch >= nchan), mem and every engine form as in nw_execute_conn.  The window is given in the
 * plan's OUTPUT samples (n_out = n / decim): the samples s_j = t0 + j * step, j = 0 .. T - 1, with
 * 0 <= t0 <= t1 <= n_out, step >= 1 (NW_E_INVALID otherwise) and T as nw_conn_time_count gives it.
 * Outputs are epoch-major:
 * NW_OUT_CROSS_SUM: out_sum complex128 (nepochs, npairs, F) = sum_j y_a conj(y_b),
 *                   out_power float64 (nepochs, nchan, F) = sum_j |y_c|^2 (may be NULL).
 * NW_OUT_PLV_SUM:   out_sum complex128 (nepochs, npairs, F) = sum_j unit phasor products;
 *                   out_power must be NULL.
 * NW_OUT_LAG_SUM:   out_sum float64 (nepochs, npairs, F, 4) = the phase-lag sums {L0 .. L3} over j;
 *                   out_power must be NULL.
 * The terms are nw_execute_conn's: fp64 values, every product and every term rounded on its own,
 * for NW_OUT_PLV_SUM each value divided by its hypot first.
 * SUMMATION ORDER (part of the contract).  There are 64 partial sums ("lanes").  Lane l starts at
 * +0.0 and adds the terms of j = l, l + 64, l + 128, ... (j < T) in that order; a lane without such
 * a j stays +0.0.  The 64 lane values are then folded: for d = 32, 16, 8, 4, 2, 1,
 * v_l <- v_l + v_{l xor d}, and v_0 is the result (v = v[:h] + v[h:] for h = 32, 16, ..., 1).  Each
 * component (re, im, each of the four lag sums, a power) is folded on its own.  A result therefore
 * depends only on its two rows and on (t0, t1, step): not on the pair list, on its tiling or on how
 * the epochs are chunked.
 * nepochs = 0 or npairs = 0: empty outputs; t0 == t1: zero sums.  The sums of all epochs live in
 * the plan (nw_stats.device_bytes); NW_E_NOMEM if they do not fit. */
int nw_execute_conn_time(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                         const int32_t* ia, const int32_t* ib, int64_t npairs,
                         int64_t t0, int64_t t1, int64_t step,
                         void* out_sum, void* out_power, int out_kind, int mem);

/* Phase-amplitude coupling: per epoch and channel pair the sums from which a comodulogram over
 * (phase scale, amplitude scale) is formed, reduced on the device along the samples of a window.
 * x, nchan, chunking (max_batch / nchan epochs, max_batch >= nchan), mem, every engine form, the
 * window (t0, t1, step) in the plan's OUTPUT samples and T are nw_execute_conn_time's.
 * ip, ia: HOST arrays [npairs], the phase and the amplitude channel of each pair (any list: repeats,
 * ip == ia).  fph [nph], fam [nam]: HOST arrays of positions into the plan's scale list (any lists:
 * repeats, a scale in both); a position outside [0, nfreq) is NW_E_INVALID.  With, in fp64,
 *   A = hypot(re, im)            of y_{e, ia[p]}[fam[k], s_j]   (amp: of channel c)
 *   u = (re / h, im / h), h = hypot(re, im)   of y_{e, ip[p]}[fph[i], s_j]   (phase: of channel c; the
 *       unit phasor of NW_OUT_PLV_SUM, NaN where |y| = 0)
 * the outputs are epoch-major:
 *   out_m     complex128 (nepochs, npairs, nph, nam) = sum_j A u
 *   out_amp   float64    (nepochs, nchan, nam, 2)    = {sum_j A, sum_j (re^2 + im^2)}   (may be NULL)
 *   out_phase complex128 (nepochs, nchan, nph)       = sum_j u                            (may be NULL)
 * Every product (A u.re, A u.im, re re, im im) and every term is rounded on its own, and every sum
 * runs in nw_execute_conn_time's SUMMATION ORDER, so a result depends only on its rows and on
 * (t0, t1, step): not on the pair list, the scale lists, their tiling or the chunks; the second
 * value of out_amp is bit-identical to nw_execute_conn_time's out_power of the same row and window.
 * nepochs = 0, npairs = 0 or an empty list: empty outputs; t0 == t1: zero sums.  The sums of all
 * epochs live in the plan (nw_stats.device_bytes); NW_E_NOMEM if they do not fit. */
int nw_execute_pac(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                   const int32_t* ip, const int32_t* ia, int64_t npairs,
                   const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam,
                   int64_t t0, int64_t t1, int64_t step,
                   void* out_m, void* out_amp, void* out_phase, int mem);

/* Phase-binned phase-amplitude coupling: per epoch, channel pair and (phase scale, amplitude scale)
 * the amplitude summed within each of nbins phase bins, reduced on the device along the samples of a
 * window: what Tort's modulation index (Tort et al. 2010), the height ratio, the preferred phase and
 * the phase-amplitude histogram are formed from.  x, ip / ia, fph / fam, nchan, chunking, mem, every
 * engine form, decimated plans, the window (t0, t1, step), T, the empty cases and NW_E_NOMEM are
 * nw_execute_pac's.  nbins must be even with 2 <= nbins <= NW_PAC_MAX_BINS (NW_E_INVALID otherwise).
 * Outputs are epoch-major:
 *   out_sum   float64 (nepochs, npairs, nph, nam, nbins) = sum_{j : bin_j = b} A_j
 *   out_count float64 (nepochs, nchan, nph, nbins)       = #{j : bin_j = b}          (may be NULL)
 * with A = hypot(re, im) of row fam[k] of channel ia[p] (nw_execute_pac's A) and bin_j the bin of row
 * fph[i] of channel ip[p] (out_count: of channel c) at sample s_j.  The counts are exact integers and
 * each row of them sums to T.
 * THE BIN (part of the contract; no atan2).  With (re, im) the row value converted to double,
 * h = nbins / 2 and (c_b, s_b) the table of nw_pac_bin_edges(nbins) -- the device reads these very
 * doubles, uploaded, and evaluates no cos or sin of its own:
 *   upper = im > 0 || (im == 0 && re > 0),  base = upper ? h : 0,
 *   bin   = base + #{k = 1 .. h - 1 : c_{base+k} im - s_{base+k} re >= 0},
 * each product rounded on its own and then subtracted (no fma), and bin = h where re == 0 && im == 0
 * (stated on its own: the count alone would put that point in bin h - 1).  Bin b holds the phases
 * [theta_b, theta_{b+1}), theta_b = -pi + 2 pi b / nbins, as floor((atan2(im, re) + pi) / (2 pi / nbins))
 * does away from the edges.  So: re < 0, im = +-0 is bin 0; y = 0 is bin h, as atan2(0, 0) = 0; a NaN
 * row value (both parts NaN, or im NaN) falls to bin 0, every comparison being false (re NaN with
 * im > 0: bin h).
 * Every sum runs in nw_execute_conn_time's SUMMATION ORDER per bin: lane l visits j = l, l + 64, ... in
 * order and adds A_j to its partial sum of bin bin_j (64 x nbins partial sums, each starting at +0.0),
 * and each bin's 64 lane values are folded with xor 32 .. 1.  A >= +0 and a partial sum is never -0.0,
 * so this is the SUMMATION ORDER applied to the terms (bin_j == b ? A_j : 0.0).  A result depends only
 * on its two rows, nbins and (t0, t1, step): not on the pair list, the scale lists, their tiling or the
 * chunks.  nw_stats.reduce_path: NW_REDUCE_PAC_BINS. */
#define NW_PAC_MAX_BINS 36
/* host-only (no GPU): cs[nbins][2] = {cos theta_b, sin theta_b}, theta_b = -pi + 2 pi b / nbins; nbins
 * as above (NW_E_INVALID otherwise, the message names the value) */
int nw_pac_bin_edges(int32_t nbins, double* cs);
int nw_execute_pac_bins(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                        const int32_t* ip, const int32_t* ia, int64_t npairs,
                        const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam,
                        int64_t t0, int64_t t1, int64_t step, int32_t nbins,
                        void* out_sum, void* out_count, int mem);

/* Time-lag surrogate statistics of nw_execute_pac's coupling (Canolty et al. 2006; tensorpac's surrogate
 * "swap amplitude time blocks"): the sum M with the amplitude cut at a sample and its two blocks swapped --
 * a circular shift inside the window -- once per listed lag, and per cell the statistics of the surrogate
 * values from which a z-score or a p-value of the observed one is formed.  All arguments, checks, chunking,
 * mem, engine forms, decimated plans, the window (t0, t1, step) and its sample count T are nw_execute_pac's.
 * lags: HOST array [nlags] of shifts in WINDOW samples, any list (repeats, 0); every lag must lie in [0, T) and
 * nlags in [0, NW_PAC_MAX_LAGS], anything else is NW_E_INVALID and the message names the value (so T = 0
 * requires nlags = 0).  centre: NW_PAC_SURR_PLAIN or NW_PAC_SURR_DEBIASED.  In fp64, with A and u as
 * nw_execute_pac defines them, indexed by the window index j = 0 .. T - 1:
 *   M_l  = sum_j A[(j + l) mod T] u[j]      every product rounded on its own, the sum in
 *                                           nw_execute_conn_time's SUMMATION ORDER on the term index j
 *   Mc_l = M_l                              (NW_PAC_SURR_PLAIN)
 *   Mc_l = M_l - D,  D = ((P.re S_A) / T, (P.im S_A) / T),  P = sum u of (ip[p], fph[i]),  S_A = sum A of
 *          (ia[p], fam[k]), each operation rounded on its own      (NW_PAC_SURR_DEBIASED: the centring of
 *          debiased_pac; the device forms P and S_A whether or not out_phase / out_amp are given)
 *   q_l  = Mc.re Mc.re + Mc.im Mc.im  (two products and one sum, each rounded),  h_l = sqrt(q_l) correctly
 *          rounded;  q_0 is that of the lag 0
 * so M_0 is bit-identical to out_m, and out_m, out_amp and out_phase are bit-identical to nw_execute_pac's.
 * The normalisations of mvl_norm and direct_pac do not change under a circular shift: one set of statistics
 * serves every measure of the same centring.  Outputs, epoch-major:
 *   out_m, out_amp, out_phase   nw_execute_pac's
 *   out_stat float64    (nepochs, npairs, nph, nam, 4)     = {sum_s h_s, sum_s q_s, #{s : q_s >= q_0}, max_s q_s},
 *            s over the list in list order; each sum starts at +0.0; the max starts at +0.0 and is replaced
 *            where q_s > max; NaN compares false                                   (NULL only if out_all is not)
 *   out_all  complex128 (nepochs, npairs, nph, nam, nlags) = M_{lags[s]} (M, not Mc)               (may be NULL)
 * A value depends only on its rows, the window and the lag list (out_all: on its own lag): not on the pair or
 * scale lists, their tiling or the chunks.  A sample with |y_p| = 0 makes that cell's sums NaN and its count
 * 0.  The regions and the staged phasors and magnitudes of one chunk (ec C (2 nph + nam) T fp64 values) live
 * in the plan (nw_stats.device_bytes); NW_E_NOMEM if they do not fit.  nw_stats.reduce_path:
 * NW_REDUCE_PAC_SURR. */
#define NW_PAC_MAX_LAGS 4096
#define NW_PAC_SURR_PLAIN 0
#define NW_PAC_SURR_DEBIASED 1
int nw_execute_pac_surr(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                        const int32_t* ip, const int32_t* ia, int64_t npairs,
                        const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam,
                        int64_t t0, int64_t t1, int64_t step,
                        const int64_t* lags, int32_t nlags, int centre,
                        void* out_m, void* out_amp, void* out_phase, void* out_stat, void* out_all, int mem);

/* Event-related phase-amplitude coupling (ERPAC; Voytek et al. 2013): nw_execute_pac's quantities
 * summed over the EPOCHS at every sample of a window instead of over the samples of every epoch -- what
 * the circular-linear correlation across epochs of the phase and the amplitude (tensorpac's
 * EventRelatedPac(method='circular')) and the across-epoch forms of nw_execute_pac's measures are formed
 * from.  x, ip / ia, fph / fam, nchan, chunking (max_batch / nchan epochs, max_batch >= nchan), mem, every
 * engine form, decimated plans, the window (t0, t1, step) in the plan's OUTPUT samples and its count T are
 * nw_execute_pac's, with the same checks.  With, in fp64, for epoch e at the window sample s_j = t0 + j step,
 *   A = hypot(re, im)                              of y_{e, ia[p]}[fam[k], s_j]   (amp: of channel c)
 *   (c, s) = (re / h, im / h), h = hypot(re, im)   of y_{e, ip[p]}[fph[i], s_j]   (phase: of channel c)
 *   u = c + i s   (nw_execute_pac's unit phasor, NaN where |y| = 0)
 * the outputs are sums over e = 0 .. nepochs - 1, the sample index j innermost:
 *   out_m     complex128 (npairs, nph, nam, T) = sum_e A u
 *   out_amp   float64    (nchan, nam, T, 2)    = {sum_e A, sum_e (re re + im im)}             (may be NULL)
 *   out_phase float64    (nchan, nph, 5, T)    = the planes sum_e c, sum_e s, sum_e c c, sum_e s s,
 *                                                sum_e c s                                      (may be NULL)
 * Every product and every term is rounded on its own (no fma into a sum).  Each output value has ONE fp64
 * accumulator that starts at +0.0 and adds the epochs' terms in epoch order, so a value depends only on
 * its rows and on its sample: not on the pair list, the scale lists, their tiling, the window or on how
 * the epochs are chunked; out_amp[..., 1] is bit-identical to nw_execute_conn's out_power of the same row
 * and sample.  nepochs = 0: zero sums; npairs = 0 or an empty list: that output is empty; t0 == t1: empty
 * outputs.  The accumulators live in the plan (nw_stats.device_bytes); NW_E_NOMEM if they do not fit,
 * NW_E_INVALID if a launch would need more than 2^31 - 1 blocks.  nw_stats.reduce_path: NW_REDUCE_ERPAC. */
int nw_execute_erpac(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                     const int32_t* ip, const int32_t* ia, int64_t npairs,
                     const int32_t* fph, int32_t nph, const int32_t* fam, int32_t nam,
                     int64_t t0, int64_t t1, int64_t step,
                     void* out_m, void* out_amp, void* out_phase, int mem);

/* Envelope correlation (Hipp et al. 2012; mne-connectivity's envelope_correlation): per epoch, channel
 * pair and scale the sums from which the Pearson correlation over time of two amplitude envelopes is
 * formed, plain or with each signal first orthogonalised against the other sample by sample, reduced
 * on the device along the samples of a window.  x, ia, ib, nchan, chunking (max_batch / nchan epochs,
 * max_batch >= nchan), mem, every engine form, decimated plans, the window (t0, t1, step) in the
 * plan's OUTPUT samples and T are nw_execute_conn_time's.  Per channel c and sample s_j, in fp64, with
 * (re, im) the row value converted to double:
 *   h = hypot(re, im),  A = h,  (ur, ui) = (re / h, im / h)
 * (the unit phasor of NW_OUT_PLV_SUM and nw_execute_pac, NaN where |y| = 0).  Outputs are epoch-major:
 * NW_ENV_PLAIN: out_pair float64 (nepochs, npairs, F)    = sum_j A_a A_b.
 * NW_ENV_ORTH:  out_pair float64 (nepochs, npairs, F, 6) = {sum u, sum u u, sum u A_b,
 *                                                           sum v, sum v v, sum v A_a} over j, with
 *   s = ua_i ub_r + (-(ua_r ub_i)),  q = |s|,  u = A_a q,  v = A_b q:
 *   u = |Im(y_a conj(y_b) / |y_b|)| is a orthogonalised against b, v is b against a.
 * both:         out_chan float64 (nepochs, nchan, F, 2)  = {sum_j A, sum_j (re re + im im)} (may be NULL).
 * Every product and every term is rounded on its own (no fma into a sum), and every sum runs in
 * nw_execute_conn_time's SUMMATION ORDER, each of the six components on its own, so a result depends
 * only on its two rows and on (t0, t1, step): not on the pair list, on its tiling or on how the epochs
 * are chunked.  The first value of out_chan is bit-identical to nw_execute_pac's out_amp[..., 0] of the
 * same row and window, the second to nw_execute_conn_time's out_power.  A sample with |y| = 0 in
 * either row makes the NW_ENV_ORTH sums of that (epoch, pair, scale) NaN, as for NW_OUT_PLV_SUM.  A
 * self pair a == b has s = 0 exactly, so its six sums are +0.0.
 * nepochs = 0 or npairs = 0: empty outputs; t0 == t1: zero sums.  The sums of all epochs live in the
 * plan (nw_stats.device_bytes); NW_E_NOMEM if they do not fit.  nw_stats.reduce_path: NW_REDUCE_ENV. */
#define NW_ENV_PLAIN 0
#define NW_ENV_ORTH  1
int nw_execute_env_time(nw_plan* plan, const void* x, int64_t nepochs, int32_t nchan,
                        const int32_t* ia, const int32_t* ib, int64_t npairs,
                        int64_t t0, int64_t t1, int64_t step,
                        void* out_pair, void* out_chan, int env_kind, int mem);

/* Shard nsig host signals over nplans plans (one per device, identical config),
 * one host thread per plan; balanced contiguous blocks (nsig / nplans signals, one
 * more for the first nsig % nplans plans).  A plan is not reentrant, so a plan
 * pointer may appear only once (NW_E_INVALID otherwise; two plans on one device are
 * fine).  For the reduction kinds each device sums its block and the host adds the
 * fp64 partial sums in device order before the mean / |.| of the result.
 * Replaces the serial per-epoch loop of EpochsWavelet.cwt (mneutils.py:39). */
int nw_execute_multi(nw_plan* const* plans, int nplans, const void* x, int64_t nsig,
                     void* out, int out_kind);

/* Device-resident sharding (one process, one host thread per device, no
 * PCIe): plan i transforms nsig[i] signals x[i] -- a DEVICE pointer on plan i's
 * device -- into out[i] (device pointer, same device, (nsig[i], F, n)).  Returns when
 * every device has finished.  Reduction kinds: each device sums its block in fp64,
 * device 0 gathers the partial sums peer-to-peer, adds them in device order and
 * writes the (F, n) result to out[0] (out[i > 0] unused).  Plans must be distinct and
 * share n, nfreq and dtype. */
int nw_execute_multi_device(nw_plan* const* plans, int nplans, const void* const* x,
                            const int64_t* nsig, void* const* out, int out_kind);

/* Shard the SCALES instead (one long signal, e.g. C5, cannot shard by
 * signal): plan i (its own device, same n / dtype / flags) holds the i-th contiguous
 * slice of the scale list, nfreq_i scales, sum nfreq_i = F.  Every device transforms all
 * nsig host signals for its scales (its own forward FFT: ~0.2 ms at 2^24, cheaper than a
 * broadcast) and writes its rows of out (nsig, F, n) -- or (F, n) for the reduction
 * kinds -- in place; no exchange.  Meant for nsig below the device count (the host
 * output is written one signal at a time). */
int nw_execute_multi_scales(nw_plan* const* plans, int nplans, const void* x, int64_t nsig,
                            void* out, int out_kind);

/* Baseline correction (base.py:18-68: class Baseline; baseline_of at 18-20) of a real
 * array x[count] (dtype NW_F32 / NW_F64).  The reference slices AXIS 0: for an array
 * whose rows hold row_len elements the baseline is rows [row0, row1) (already
 * normalised like a Python slice), i.e. the contiguous elements [row0*row_len,
 * row1*row_len).  basemean = its mean and std = its population std (np.std), both over
 * all of its elements, are reduced on the device in fp64; then out[i] = op(x[i]) in the
 * array's precision:
 *   NW_BL_MEAN    x - basemean                 (base.py:53-54)
 *   NW_BL_RATIO   x / basemean                 (56-57)
 *   NW_BL_PERCENT (x - basemean) / basemean    (59-60)
 *   NW_BL_LOG     log10(x / basemean)          (62-63)
 *   NW_BL_ZSCORE  (x - basemean) / std         (65-66)
 *   NW_BL_ZLOG    log10(x / basemean) / std    (68-69)
 * mem = NW_MEM_HOST (synchronous) or NW_MEM_DEVICE (pointers on `device`, synchronous
 * on the device's null stream).  stats (optional, host) receives {basemean, std}.
 * An empty baseline gives NaN statistics, like numpy. */
#define NW_BL_MEAN    0
#define NW_BL_RATIO   1
#define NW_BL_PERCENT 2
#define NW_BL_LOG     3
#define NW_BL_ZSCORE  4
#define NW_BL_ZLOG    5
int nw_baseline(int device, int dtype, const void* x, int64_t count, int64_t row_len, int64_t row0,
                int64_t row1, int op, void* out, int mem, double* stats);

/* Time-domain wavelets of the stock kinds, make_wavelet(s) (base.py:346-376), computed on
 * `device`: one row per freq, complex128, left-aligned in out[nfreq][*max_len] (host).
 *   NW_MORSE {b, r}, NW_SHANNON {}  (WaveletMode.Reverse): ifft of the spectrum (its
 *     default freq = 1) on np.arange(0, sfreq/f*real_wave_length, 1/f), then the centre
 *     slice [m//2, m//2*3) of hstack(conj(flip(w)), w)  -> 2*(m//2) points;
 *   NW_MORLET {sigma, gabor[, c, k]}, NW_MEXICAN_HAT {sigma}, NW_HAAR {}: the time-domain
 *     formula on np.arange(-T/2, T/2, step) of _setup_waveletshape (base.py:196-216).
 * row_len[nfreq] receives each row's length.  out == NULL: lengths only (to size out). */
int nw_make_wavelets(int device, int kind, const double* params, int nparams, const double* freqs, int nfreq,
                     double sfreq, double real_wave_length, void* out, int64_t* max_len, int64_t* row_len);

/* Page-locked host memory for results (no reference counterpart: the drop-in classes pool
 * their result arrays in it, ninwavelets_amd/engine.py HostPool).  nw_execute with
 * NW_MEM_HOST writes an output that lies inside such an allocation by DMA directly, without
 * the staging copy; a fresh pageable array instead is faulted in page by page during the
 * copy-out.  nw_host_free takes exactly a pointer nw_host_alloc returned. */
int nw_host_alloc(int64_t bytes, void** ptr);
int nw_host_free(void* ptr);
/* Advise a pageable host buffer the CALLER has just allocated for a result onto transparent
 * huge pages (madvise MADV_HUGEPAGE over its whole 2 MiB pages; no reference counterpart:
 * the drop-in classes call it for the fresh arrays they return when the page-locked pool is
 * full, ninwavelets_amd/engine.py).  A fresh array is then faulted in 2 MiB at a time during
 * the copy-out instead of 4 KiB.  nw_execute never changes the page policy of the memory it
 * is handed.  *advised (may be NULL) receives the bytes advised (0 below one huge page). */
int nw_host_advise(void* ptr, int64_t bytes, int64_t* advised);

int nw_plan_set_stream(nw_plan* plan, void* hip_stream);   /* NULL: the plan's own stream */
/* The hipStream_t the plan currently launches on (for event ordering with the caller's
 * streams: device-buffer executes are asynchronous on it). */
int nw_plan_get_stream(nw_plan* plan, void** hip_stream);
int nw_plan_sync(nw_plan* plan);
int nw_plan_stats(nw_plan* plan, nw_stats* stats);
int nw_plan_reset_stats(nw_plan* plan);
int nw_plan_destroy(nw_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* NINWAVE_H */
