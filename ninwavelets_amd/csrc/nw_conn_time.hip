// nw_conn_time.hip — over-time connectivity (nw_execute_conn_time): the complex rows of a chunk of
// epochs x channels reduced along the SAMPLE axis into one value per epoch, channel pair and scale.
//
//   src [((e * C + c) * F + f) * n_out + t]   complex T: the chunk's rows, epoch-major
//   sum [(e * P + p) * F + f]                 complex fp64: S_e,p (PLV: Phi_e,p), p = (ia[p], ib[p])
//   SUM_LAG: sum [((e * P + p) * F + f) * 4 ..] fp64 {L0, L1, L2, L3}
//   power [(e * C + c) * F + f]               fp64: P_e,cc (nw_conn_time_power_kernel)
// each the sum over the window's samples s_j = t0 + j * step, j = 0 .. T - 1, of the terms
// nw_conn_accumulate_kernel (nw_conn.hip) adds per epoch: fp64 values, every product and every term
// rounded on its own (no fma into a sum), for PLV each value divided by its hypot first.
//
// Summation order (the contract, ninwave.h; nw_shape.h conn_time_lane): lane l starts every
// accumulator at +0.0 and adds the terms of j = l, l + 64, l + 128, ... in that order; lanes and tail
// samples without a j < T add nothing.  The 64 lane values are then folded, v_l <- v_l + v_{l xor d}
// for d = 32, 16, 8, 4, 2, 1, every component on its own, and lane 0 writes the result.  A result
// depends only on its two rows and on (t0, T, step): not on the pair list, the tiling or the chunks.
//
// nw_conn_time_kernel is the skeleton pair_time_sums of nw_reduce_dev.h (a block owns one epoch of the
// chunk, one scale and one pair tile; lane = sample; double-buffered staging over sample tiles) with the
// SUM_* policies nw_conn_accumulate_kernel uses; nw_conn_time_power_kernel is its row_time_sums.
#include <algorithm>

#include "nw_reduce_dev.h"

namespace nw {
namespace {

// the skeleton pair_time_sums (nw_reduce_dev.h) with the SUM_* arithmetic nw_conn_accumulate_kernel uses
template <typename T, int MODE>
__global__ __launch_bounds__(kConnThreads) void nw_conn_time_kernel(
    const cplx<T>* __restrict__ src, double2* __restrict__ sum, const ConnTile* __restrict__ tiles, int ntiles,
    int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0, int64_t count, int64_t step, int xcd) {
    pair_time_sums<SumPolicy<MODE>>(src, sum, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, t0, count, step, xcd);
}

// power[(e * C + c) * F + f] = sum_j |y_{e,c}[f, s_j]|^2: one wave per row (row_time_sums), the order of the contract
template <typename T>
__global__ __launch_bounds__(kConnThreads) void nw_conn_time_power_kernel(const cplx<T>* __restrict__ src,
                                                                         double* __restrict__ power, int64_t nrows,
                                                                         int64_t n_out, int64_t t0, int64_t count,
                                                                         int64_t step) {
    row_time_sums<kConnWaves>(
        src, nrows, nrows * n_out, n_out, t0, count, step, [&](int64_t row) { return row * n_out; },
        [](int64_t, double& p, double&, double re, double im) { p = add_nc(p, power_term(re, im)); },
        [&](int64_t row, double p, double) { power[row] = p; });
}

}  // namespace

hipError_t launch_conn_time(int dtype, int mode, const void* src, void* sum, double* power, const ConnTile* tiles,
                            int ntiles, int64_t ec, int nchan, int nfreq, int64_t n_out, int64_t npairs, int64_t t0,
                            int64_t count, int64_t step, bool xcd, hipStream_t s) {
    const int64_t blocks = ntiles > 0 ? conn_time_blocks(ec, nfreq, ntiles, xcd) : 0;
    const int64_t nrows = ec * nchan * nfreq;
    const int64_t pb = (nrows + kConnWaves - 1) / kConnWaves;
    if (blocks > 0x7fffffff || pb > 0x7fffffff) return hipErrorInvalidValue;
    for_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (blocks > 0)
            for_sum_mode(mode, [&](auto v) {
                nw_launch(nw_conn_time_kernel<T, decltype(v)::value>, dim3((unsigned)blocks), dim3(kConnThreads), 0, s,
                          (const cplx<T>*)src, (double2*)sum, tiles, ntiles, ec, nchan, nfreq, n_out, npairs, t0, count,
                          step, xcd ? 1 : 0);
            });
        if (power && mode == SUM_CROSS && pb > 0)
            nw_launch(nw_conn_time_power_kernel<T>, dim3((unsigned)pb), dim3(kConnThreads), 0, s, (const cplx<T>*)src,
                      power, nrows, n_out, t0, count, step);
    });
    return hipGetLastError();
}

}  // namespace nw
