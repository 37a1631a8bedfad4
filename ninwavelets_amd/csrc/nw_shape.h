// nw_shape.h — launch geometry of the on-chip engines: the rules that decide which kernel
// instantiation runs a row and which block computes it.  Integer arithmetic only (no device
// pointer is read), shared by the kernels and their launchers and compiled by the host
// compiler too: tests/asan/host_asan.cpp checks it exhaustively on a CPU (mode `self`) and
// prints it for comparison with the tests' Python restatement (mode `shapes`).
//   - the XCD-aware block mapping (block_slot) and its host-side inverse (block_grid);
//   - the one-pass size table (fused_e), its visitor and the decimated lengths;
//   - block shapes (signals per block, XCD tiles) of the one-pass kernels;
//   - the W-table layout, the support rounding and the pass-0 ladders;
//   - which partial-sum kernels exist.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ninwave.h"

#ifdef __HIP__
#define NW_SHAPE_HD __host__ __device__
#else
#define NW_SHAPE_HD
#endif
#define NW_INLINE inline __attribute__((always_inline))

namespace nw {

template <typename T> constexpr int kDtypeOf = sizeof(T) == 4 ? NW_F32 : NW_F64;

// ---- block mapping ----------------------------------------------------------------------

// XCD-aware block -> (scale, signal group).  Blocks b, b+8, b+16, ... share an XCD
// (and its 4 MiB L2); the ~64 of them resident at a time cover a tile of
// kTileF scales x kTileG signal groups, so each W row is read by kTileG blocks
// and each X group by kTileF blocks from L2 (W + X of a tile ~2.5 MiB), and
// the XCD sweeps all scales of its groups before moving on.
// (nrows: the launch's scales; a slot with row >= nrows or group beyond the launch's groups is
// padding and its block returns.)
struct BlockSlot {
    int row, group;
};
NW_SHAPE_HD NW_INLINE BlockSlot block_slot(int b, int nrows, int tile_f, int tile_g) {
    const int xcd = b & 7;
    const int local = b >> 3;
    const int pos = local % (tile_f * tile_g);
    const int round = local / (tile_f * tile_g);
    const int nfr = (nrows + tile_f - 1) / tile_f;
    return {(round % nfr) * tile_f + pos % tile_f, ((round / nfr) * tile_g + pos / tile_f) * 8 + xcd};
}

// ... and at most as many groups as a launch has (in units of 8 XCD slots): C2 (64 signals =
// 8 groups) with 4-group tiles padded its grid to 4x its real blocks
NW_SHAPE_HD constexpr int tile_g_of(int64_t nsg, int tg_max) {
    const int64_t per = (nsg + 7) / 8;
    return per < tg_max ? (int)(per < 1 ? 1 : per) : tg_max;
}

// The grid whose blocks block_slot maps onto nrows x groups: groups padded to whole tiles
// (8 XCDs x tile_g), rows to whole tile_f.  ok: the grid and the padded group count fit the
// kernels' 32-bit block and group indices.  A kernel and its launcher must agree on
// (tile_f, tile_g): where they do not, rows are left unwritten or written twice.
struct BlockGrid {
    int tile_g;
    int64_t groups_pad, blocks;
    bool ok;
};
constexpr BlockGrid block_grid_tile(int64_t groups, int nrows, int tile_f, int tile_g) {
    const int64_t groups_pad = (groups + 8 * tile_g - 1) / (8 * tile_g) * (8 * tile_g);
    const int64_t nfr = (nrows + tile_f - 1) / tile_f;
    const int64_t blocks = groups_pad * nfr * tile_f;
    return {tile_g, groups_pad, blocks, blocks <= 0x7fffffff && groups_pad <= 0x7fffffff};
}
// ... with the tile narrowed to the launch (tile_g_of): the kernel takes tile_g as an argument
constexpr BlockGrid block_grid(int64_t groups, int nrows, int tile_f, int tile_g_max) {
    return block_grid_tile(groups, nrows, tile_f, tile_g_of(groups, tile_g_max));
}

// XCD tiles of the chirp-z kernel (nw_chirp.hip) and of the two-pass row kernel (nw_large.hip),
// fixed per kernel (block_grid_tile)
constexpr int kTileFC = 8;    // scales per XCD tile
constexpr int kTileGC = 4;    // signal groups per XCD tile
constexpr int kRowTileF = 8;      // scales per XCD tile
constexpr int kRowTileG = 8;      // row groups per XCD tile

// ---- the one-pass size table --------------------------------------------------------------

// Elements per thread E of each fused size (threads = n / E).  Measured: fp32 n = 4096 at
// E = 32 slower (0.350 -> 0.404 ms power); n = 8192 at E = 32 vs 16: power 0.887 -> 0.768 ms,
// cwt 1.034 -> 0.926; fp64 at n >= 8192: E = 32 (3 passes, 256 VGPRs, 2 waves/SIMD) vs E = 16
// (4 passes): 8192 cwt 2.907 -> 2.573 ms, power 2.397 -> 1.991; 16384 cwt 3.447 -> 3.124,
// power 2.615 -> 2.312 (256 x 256 rows; 128 x 256 at 16384).
// power-of-two n: 2^10..2^14 in fp32 and fp64 (fp64 at 8192 / 16384: E = 32 with 256 VGPRs,
// W re-read per signal); 0: not a one-pass size
constexpr int kFusedLog2Min = 10, kFusedLog2Max = 14;
constexpr int fused_e(int64_t n, int dtype) {
    if (dtype != NW_F32 && dtype != NW_F64) return 0;
    if (n < (1 << kFusedLog2Min) || n > (1 << kFusedLog2Max) || (n & (n - 1))) return 0;
    return n <= 4096 ? 16 : 32;
}
constexpr bool fused_supported(int64_t n, int dtype) { return fused_e(n, dtype) != 0; }

// Transform lengths ND = n / decim of the decimated kernel (nw_decim.hip): the table's rows
// for 1024 <= ND <= 8192, at the same E.
// power-of-two n = 2048 .. 16384 and decim >= 2 with n / decim >= 1024, fp32 and fp64: ten
// (n, decim) pairs per dtype
constexpr int64_t kDecimMaxND = 8192;
constexpr bool decim_supported(int64_t n, int dtype, int decim) {
    if (decim < 2 || (decim & (decim - 1))) return false;
    return fused_supported(n, dtype) && fused_supported(n / decim, dtype) && n / decim <= kDecimMaxND;
}

// One visitor over the table: f(FusedSize<T, N, E>{}) for the row of (n, dtype), `miss` past it.
template <typename T, int N, int E> struct FusedSize {};
template <typename T, int LG, typename R, typename F>
inline R for_fused_length(int64_t n, R miss, F& f) {
    if constexpr (LG > kFusedLog2Max) {
        return miss;
    } else {
        if (n == (1 << LG)) return f(FusedSize<T, (1 << LG), fused_e(1 << LG, kDtypeOf<T>)>{});
        return for_fused_length<T, LG + 1>(n, miss, f);
    }
}
template <typename R, typename F>
inline R for_fused_size(int64_t n, int dtype, R miss, F f) {
    if (dtype == NW_F32) return for_fused_length<float, kFusedLog2Min>(n, miss, f);
    if (dtype == NW_F64) return for_fused_length<double, kFusedLog2Min>(n, miss, f);
    return miss;
}

// ---- block shapes of the one-pass kernels ---------------------------------------------------

// Signals per partial-sum row: the block size of both the fused kernels (kGroup) and the
// chirp-z kernel (kGroupC), each static_assert'ed equal to it, so one fused_psum_groups sizes
// and accumulates the partial rows of either form
constexpr int kPsumGroup = 8;

// signals per block: C3 0.354 -> 0.348 ms, C4 1.774 -> 1.770 vs 4 (2 and 16 slower or equal).
// fp64 (one block per CU): 8 since round 6 (C4 shape fp64 7.31-7.32 -> 7.25-7.28 ms per launch,
// with the fine pass-0 variants below 7.21-7.24; 2 signals +2.6 %, tiles 4 x 8 +1.5 %, 8 x 2
// +0.3 %; profiles/r06_f64_group_ab.txt).  Round 3 had taken 4 (then 10.04 -> 9.66 ms against
// 8 signals, when X was re-read from L2 per scale without the LDS-DMA)
constexpr int kGroup = 8;
static_assert(kGroup == kPsumGroup, "fused partial rows are counted by fused_psum_groups");
// (-DNW_GROUP64 / NW_TILE64_F / NW_TILE64_G: diagnostic A/B of the fp64 block and tile shape)
#ifndef NW_GROUP64
#define NW_GROUP64 8
#endif
constexpr int kGroup64 = NW_GROUP64;
// XCD tile: kTileF scales x kTileG signal groups per XCD round (fp64 tiles 16 x 2, 4 x 8,
// 32 x 1, 2 x 16 measured -2.4 / -0.2 / -4.8 / -3.5 % against 8 x 4)
constexpr int kTileF = 8, kTileG = 4;
#ifndef NW_TILE64_F
#define NW_TILE64_F kTileF
#endif
#ifndef NW_TILE64_G
#define NW_TILE64_G kTileG
#endif
template <typename T> constexpr int kTileFT = sizeof(T) == 8 ? NW_TILE64_F : kTileF;
template <typename T> constexpr int kTileGT = sizeof(T) == 8 ? NW_TILE64_G : kTileG;
// fp64 output kernels at n = 16384 (one block per CU): 16-signal blocks in XCD tiles of 8 scales
// x 2 groups -- the same X + W working set per XCD round as 8 x 4 of 8 signals, half the blocks
// (C4 shape fp64 7.175 -> 7.12-7.13 and 7.246 -> 7.212 ms per launch on two boxes, -0.5 %;
// 32 x 1 -0.3 %, 16 signals in 8 x 4 tiles -0.4 %, 16 in 8 x 1 +-0; profiles/r06_f64_g16_ab.txt).
// Smaller n (two blocks per CU) and the partial-sum kernels keep kGroup64 / kTileGT.
#ifndef NW_GROUP64_16K
#define NW_GROUP64_16K 16
#endif
#ifndef NW_TILE64_G_16K
#define NW_TILE64_G_16K 2
#endif
template <typename T, int N> constexpr int kGroupOut = sizeof(T) == 8 ? (N == 16384 ? NW_GROUP64_16K : kGroup64) : kGroup;
template <typename T, int N> constexpr int kTileGOut = sizeof(T) == 8 && N == 16384 ? NW_TILE64_G_16K : kTileGT<T>;

// Signals per block of the output kernels: `base`, halved (to 2) while a launch would fill the
// chip fewer than kMinRounds times over (512 resident 512-thread blocks): a small launch (C2:
// 64 signals x 128 scales = 1024 blocks of 8, two rounds) otherwise ends on a tail of long
// blocks.
constexpr int64_t kMinRounds = 4, kResidentBlocks = 512;
constexpr int group_filling(int base, int64_t nsig, int nfreq) {
    int g = base;
    while (g > 2 && (nsig + g - 1) / g * (int64_t)nfreq < kMinRounds * kResidentBlocks) g /= 2;
    return g;
}

// ---- the W table ------------------------------------------------------------------------------

// bytes of the W rows in the table buffer (the wnz[nfreq] support array follows them)
constexpr size_t wtab_row_bytes(int64_t n, int nfreq, size_t esz, bool realw) {
    const size_t b = (size_t)n * nfreq * esz * (realw ? 1 : 2);
    return (b + 15) / 16 * 16;
}
// ... and that array (esz: bytes of the real type; realw: real rows, complex for table wavelets)
inline const int* wtab_wnz(const void* wtab, int64_t n, int nfreq, size_t esz, bool realw) {
    return reinterpret_cast<const int*>(static_cast<const char*>(wtab) + wtab_row_bytes(n, nfreq, esz, realw));
}

// wnz of a row whose pass-0 elements 0 .. need-1 can be nonzero (wsupport_kernel): the
// next power of two up to 4, then the next multiple
// of 4 (the pass-0 variants: NZ = 4, 8, 12, 16 at E = 16; 4, 8, 12, 16, 20, 24, 32 at E = 32
// fp32; a multiple of 2^WSH, so nz >> WSH is exact for the partial-sum kernels' smaller E).
// Rows pruned in steps of 4 elements: C3 1.205 -> 1.186 ms per launch (NZ = 12 at E = 16).
NW_SHAPE_HD constexpr int wnz_round(int need, int e) {
    int p2 = 1;
    while (p2 < need && p2 < 8) p2 <<= 1;
    if (p2 < need) p2 = (need + 3) / 4 * 4;
    return p2 < e ? p2 : e;
}

// ---- pass-0 variants --------------------------------------------------------------------------

// E = 32: a pass-0 variant for rows whose support ends below 3/4 of n (NZ = 24: C4's rows
// above 186 Hz), between the power-of-two variants: C4 3.360-3.368 -> 3.346-3.351 ms
constexpr bool kNz24 = true;
template <typename T, int N, int E> constexpr bool kNz24Of = kNz24 && E > 16;
// NZ = 12 and 20 between them (fp32 only: fp64 n = 16384 |y| spills 20 B with them)
template <typename T, int N, int E> constexpr bool kNzFineOf = kNz24Of<T, N, E> && sizeof(T) == 4;
// ... and for the fp64 cwt output (round 6: C4 shape fp64 -0.7 to -0.9 %; its |y| spills with
// them; -DNW_F64_FINE=0 for the A/B)
#ifndef NW_F64_FINE
#define NW_F64_FINE 1
#endif
#if NW_F64_FINE
template <typename T, int N, int E, int OUT> constexpr bool kNzFineOut = kNzFineOf<T, N, E> ||
    (kNz24Of<T, N, E> && OUT == NW_OUT_CWT);
#else
template <typename T, int N, int E, int OUT> constexpr bool kNzFineOut = kNzFineOf<T, N, E>;
#endif
// The pass-0 variant (elements read and multiplied per thread) that runs a row of support nz:
// the smallest instantiated NZ >= nz.  The X LDS-DMA copies what THAT variant reads (a row
// of support 12 on a kernel without the NZ = 12 variant runs NZ = 16, which reads 16 elements)
// (E, FINE = kNzFineOut, NZ24 = kNz24Of at compile time: the kernels' ladder is a few scalar compares)
template <int E, bool FINE, bool NZ24>
NW_SHAPE_HD constexpr NW_INLINE int pass0_variant(int nz) {
    if (nz <= 4) return 4;
    if (nz <= 8) return 8;
    if (FINE && nz <= 12) return 12;
    if (E > 16 && nz <= 16) return 16;
    if (FINE && nz <= 20) return 20;
    if (NZ24 && nz <= 24) return 24;
    return E;
}
// the signal-pair kernel's ladder (E = 16): NZ = 4, 8, 12, E (nw_fused_pair_kernel's dispatch)
NW_SHAPE_HD constexpr int pair_pass0_variant(int nz, int e) { return nz <= 4 ? 4 : nz <= 8 ? 8 : nz <= 12 ? 12 : e; }

// ---- which kernel runs ----------------------------------------------------------------------

// signal pairs (nw_fused_pair_kernel): fp32, E = 16, analytic real W rows
template <typename T, int E, bool REALW>
constexpr bool kPairMode = std::is_same<T, float>::value && E <= 16 && REALW;

// epoch power / phase partials: analytic rows; fp32 power to E = 32, fp32 phases and fp64 at E = 16
// Elements per thread of the partial-sum kernels (EO: the output kernels'): fp32 power keeps
// EO (E = 32 at n = 8192 / 16384: E fp64 accumulators at 2 waves/SIMD); fp32 phases (2E fp64
// accumulators) and fp64 (the drop-in's default dtype, 2 waves/SIMD already at 256 VGPRs)
// run at E = 16 -- n = 8192 / 16384 then take 512 / 1024 threads, the W-support table
// shifted by log2(EO / 16) (nw_fused_kernel's WSH)
template <typename T, int EO, bool PHASE>
constexpr int kPsE = (EO >= 32 && (PHASE || sizeof(T) == 8)) ? 16 : EO;
template <int EO, int E> constexpr int kPsShift = EO == E ? 0 : EO == 2 * E ? 1 : 2;
// combinations whose accumulators fit without spilling (tools/regs.py): at 1024 threads
// (n = 16384, E = 16) a wave has 128 VGPRs, and neither fp64 power (228 B of scratch) nor
// phases (fp32: 84 B) fit there -- n = 16384 keeps the chunk path for those
template <typename T, int N, int EO>
constexpr bool kPSumOK = !(sizeof(T) == 8 && N / kPsE<T, EO, false> > 512);
template <typename T, int N, int EO>
constexpr bool kPhSumOK = N / kPsE<T, EO, true> <= 512;

}  // namespace nw
