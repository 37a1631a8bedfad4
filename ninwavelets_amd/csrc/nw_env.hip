// nw_env.hip — envelope correlation (nw_execute_env_time): the complex rows of a chunk of epochs x
// channels reduced along the SAMPLE axis into the Pearson sums of two amplitude envelopes per epoch,
// channel pair and scale, plain or pairwise orthogonalised (Hipp et al. 2012).
//
//   src  [((e * C + c) * F + f) * n_out + t]     complex T: the chunk's rows, epoch-major
//   NW_ENV_PLAIN: pair [(e * P + p) * F + f]           fp64: sum_j A_a A_b,       p = (ia[p], ib[p])
//   NW_ENV_ORTH:  pair [((e * P + p) * F + f) * 6 ..]  fp64 {sum u, sum u u, sum u A_b, sum v, sum v v, sum v A_a}
//   chan [((e * C + c) * F + f) * 2 ..]          fp64 {sum_j A, sum_j (re re + im im)}  (nw_env_chan_kernel)
// over the window's samples s_j = t0 + j * step, j = 0 .. T - 1, with, in fp64 per channel and sample,
//   h = hypot(re, im),  A = h,  (ur, ui) = (re / h, im / h)
// (SUM_PLV's and nw_pac.hip's unit phasor, NaN where |y| = 0) and per pair and sample
//   s = ua_i ub_r + (-(ua_r ub_i)),  q = |s|,  u = A_a q,  v = A_b q:
// u = |Im(y_a conj(y_b) / |y_b|)|, a orthogonalised against b, and v the reverse.  Every product and
// every term is rounded on its own (no fma into a sum).  A self pair has s = +0.0 exactly.
//
// Summation order: that of nw_execute_conn_time (nw_shape.h conn_time_lane): lane l starts at +0.0 and
// adds the terms of j = l, l + 64, ... in that order, the 64 lane values are folded with xor 32 .. 1,
// every component on its own, and lane 0 writes.  A result depends only on its two rows and on
// (t0, T, step): not on the pair list, the tiling or the chunks.
//
// nw_env_time_kernel is the skeleton pair_time_sums of nw_reduce_dev.h, which nw_conn_time_kernel shares,
// with the policies EnvPlain and EnvOrth: per sample tile the tile's channels are staged once in LDS as
// {A, ur, ui} (plain: A), so the hypot and the two divisions are paid once per channel and sample and not
// once per pair.  NW_ENV_ORTH keeps 6 fp64 accumulators for each of its 16 pairs in registers (192 of the
// block's 512 per lane; no scratch: profiles/r17_env_rate.txt) and stages 48 KiB (plain: 16).
// nw_env_chan_kernel is its row_time_sums.  The diagnostic switches NW_ABL_ENV_NOLOAD and
// NW_ABL_ENV_NODIV (tools/env_rate.py) live with the code they cut, in the header.
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

// the skeleton pair_time_sums (nw_reduce_dev.h) with the envelope arithmetic (EnvPlain, EnvOrth)
template <typename T, int MODE>
__global__ __launch_bounds__(kConnThreads) void nw_env_time_kernel(
    const cplx<T>* __restrict__ src, double* __restrict__ pair, const ConnTile* __restrict__ tiles, int ntiles,
    int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0, int64_t count, int64_t step, int xcd) {
    static_assert(MODE == NW_ENV_PLAIN || MODE == NW_ENV_ORTH, "envelope mode");
    using P = std::conditional_t<MODE == NW_ENV_ORTH, EnvOrth, EnvPlain>;
    static_assert(P::kOut == env_pair_values(MODE), "fp64 values per epoch, pair and scale in `pair`");
    pair_time_sums<P>(src, pair, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, t0, count, step, xcd);
}

// chan[(e * C + c) * F + f] = {sum_j A, sum_j |y|^2} of the row: one wave per row (row_time_sums), the
// order of the contract; the first sum as nw_pac_rows_kernel forms its amplitude sum, the second as
// nw_conn_time_power_kernel forms its power
template <typename T>
__global__ __launch_bounds__(kConnThreads) void nw_env_chan_kernel(const cplx<T>* __restrict__ src,
                                                                   double* __restrict__ chan, int64_t nrows,
                                                                   int64_t n_out, int64_t t0, int64_t count,
                                                                   int64_t step) {
    row_time_sums<kConnWaves>(
        src, nrows, nrows * n_out, n_out, t0, count, step, [&](int64_t row) { return row * n_out; },
        [](int64_t, double& s0, double& s1, double re, double im) {
            s0 = add_nc(s0, hypot(re, im));
            s1 = add_nc(s1, power_term(re, im));
        },
        [&](int64_t row, double s0, double s1) {
            chan[2 * row] = s0;   // (8-aligned only: the sums follow the NW_ENV_PLAIN pair sums)
            chan[2 * row + 1] = s1;
        });
}

}  // namespace

hipError_t launch_env_time(int dtype, int env, const void* src, void* pair, double* chan, const ConnTile* tiles,
                           int ntiles, int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0,
                           int64_t count, int64_t step, bool xcd, hipStream_t s) {
    const int64_t blocks = ntiles > 0 ? conn_time_blocks(ec, nfreq, ntiles, xcd) : 0;
    const int64_t nrows = ec * nchan * nfreq;
    const int64_t cb = (nrows + kConnWaves - 1) / kConnWaves;
    if (blocks > 0x7fffffff || cb > 0x7fffffff) return hipErrorInvalidValue;
    if (env != NW_ENV_PLAIN && env != NW_ENV_ORTH) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        auto go = [&](auto v) {
            nw_launch(nw_env_time_kernel<T, decltype(v)::value>, dim3((unsigned)blocks), dim3(kConnThreads), 0, s,
                      (const cplx<T>*)src, (double*)pair, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, t0, count, step,
                      xcd ? 1 : 0);
        };
        if (blocks > 0) {
            if (env == NW_ENV_ORTH) go(std::integral_constant<int, NW_ENV_ORTH>{});
            else go(std::integral_constant<int, NW_ENV_PLAIN>{});
        }
        if (chan && cb > 0)
            nw_launch(nw_env_chan_kernel<T>, dim3((unsigned)cb), dim3(kConnThreads), 0, s, (const cplx<T>*)src,
                      chan, nrows, n_out, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
