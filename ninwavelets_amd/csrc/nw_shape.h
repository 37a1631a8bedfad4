// nw_shape.h — launch geometry of the on-chip engines: the rules that decide which kernel
// instantiation runs a row and which block computes it.  Integer arithmetic only (no device
// pointer is read), shared by the kernels and their launchers and compiled by the host
// compiler too: tests/asan/host_asan.cpp checks it exhaustively on a CPU (mode `self`) and
// prints it for comparison with the tests' Python restatement (mode `shapes`).
//   - the XCD-aware block mapping (block_slot) and its host-side inverse (block_grid);
//   - the one-pass size table (fused_e), its visitor and the decimated lengths;
//   - block shapes (signals per block, XCD tiles) of the one-pass kernels;
//   - the W-table layout, the support rounding and the pass-0 ladders;
//   - which partial-sum kernels exist;
//   - the connectivity kernel (nw_conn.hip): its pair tile, sample tile and block order;
//   - the over-time connectivity kernel (nw_conn_time.hip): its block -> (epoch, scale, pair tile)
//     map, block count, the sample count of a window and the lane of a sample (the order contract);
//   - the phase-amplitude coupling kernel (nw_pac.hip): its scale tile, the tile counts and its
//     block -> (epoch, pair, phase tile, amplitude tile) map;
//   - the surrogate kernels of the coupling (nw_pac_surr.hip): the layout of the staged unit phasors and
//     magnitudes, the staging launch's blocks, the circular shift and the lane of a cell;
//   - the event-related coupling kernel (nw_erpac.hip): its sample-tile count, its block -> (pair,
//     sample tile, phase tile, amplitude tile) map and its block count;
//   - the phase-binned coupling kernel (nw_pac_bins.hip): the geometry chosen from nbins, its LDS
//     bytes and its tile counts;
//   - the two-pass engine (nw_large.hip): the (N1, N2) split and its visitor, the row pass's
//     elements per thread, rows per block, pass-0 ladder and LDS-DMA rule, the column pass's
//     block shape, the scale chunk and the support buffer's layout (mode `large` prints them);
//   - the chirp-z engine (nw_chirp.hip): the (dtype, M, E) table and its visitor, the lengths
//     it takes and a row's M class.
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

// cross-channel pair reductions (nw_execute_pair: NW_OUT_CROSS_SUM / NW_OUT_PLV_SUM): the
// (n, dtype, wavelet kind, out_kind) whose sums are formed as block partials inside
// nw_fused_pair_kernel.  The candidates are fp32, n = 1024 / 2048 / 4096, analytic rows; an
// instantiation enters only with 0 B of scratch and a measured rate no lower than the chunk
// path's (k_accumulate_pair over the chunk's complex rows).  All six hold both
// (profiles/r11_pair_rate.txt, r11_pair_isa.txt).
template <int N> constexpr bool kPairXSumOK = N >= 1024 && N <= 4096;     // 4E fp64 accumulators, 2 waves/SIMD
template <int N> constexpr bool kPairPlvSumOK = N >= 1024 && N <= 4096;   // 2E fp64 accumulators, 2 waves/SIMD
constexpr bool pair_partials_supported(int64_t n, int dtype, int kind, int out_kind) {
    if (dtype != NW_F32 || (kind != NW_MORSE && kind != NW_MORLET && kind != NW_SHANNON)) return false;
    const bool xs = n == 1024 ? kPairXSumOK<1024> : n == 2048 ? kPairXSumOK<2048> : n == 4096 ? kPairXSumOK<4096> : false;
    const bool ps = n == 1024 ? kPairPlvSumOK<1024> : n == 2048 ? kPairPlvSumOK<2048> : n == 4096 ? kPairPlvSumOK<4096> : false;
    return out_kind == NW_OUT_CROSS_SUM ? xs : out_kind == NW_OUT_PLV_SUM ? ps : false;
}

// ---- lane-addressed exchange images (fp32, n = 16384, E = 32) ---------------------------------

// The two LDS exchanges of the fp32 n = 16384 one-pass kernels (512 threads, passes of radix
// 32, 32, 16) laid out so that every wave store is 64 consecutive dwords from a wave-uniform
// base: ds_write_addtid_b32 (address M0 + offset + 4 * lane, no address VGPR, 2 LDS cycles per
// dword and wave against 6-13 for the 8- and 16-byte stores of the padded images).  Slot indices
// i are those of the padded images (nw_fft_dev.h lds_write / lds_read): only the address of a
// slot changes, not which value it holds.
//   0 -> 1: slot i = 32 t + p (thread t's output p)            -> dword p * S1 + t
//           read by butterfly u, element r as slot u + 512 r    =  (u % 32) * S1 + u / 32 + 16 r
//   1 -> 2: slot i = (j / 32) * 1024 + j % 32 + 32 i' (butterfly j's output i')
//                                                               -> dword i' * S2 + j
//           read by butterfly j2, element r as slot j2 + 1024 r =  (j2 / 32) * S2 + j2 % 32 + 32 r
// S1 = 513: a 32-lane ds_read_b32 group (u = 32 g + l) hits bank l + g + const, each once.
// S2 = 544 = 32 mod 64: lanes 0-15 of a ds_read_b64 group (pairs j2 = 2t, 2t + 1) cover dwords
// 0-31 of one row and lanes 16-31 those of the next, 32 banks on: the 64 banks once, without
// the lane remap the padded image needs there (PassInfo::SWZ).
// -DNW_LANE_IMAGE=0: the padded images everywhere (diagnostic A/B).
#ifndef NW_LANE_IMAGE
#define NW_LANE_IMAGE 1
#endif
template <typename T, int N, int E>
constexpr bool kLaneImageShape = NW_LANE_IMAGE && std::is_same<T, float>::value && N == 16384 && E == 32;
namespace lane_image {
constexpr int kN = 16384, kE = 32, kT = kN / kE;   // threads = butterflies of pass 1
constexpr int kS1 = 513, kS2 = 544;                // row strides in dwords
constexpr int kElems = kE * kS2;                   // dwords of the image region (both images fit)
constexpr int kBytes = kElems * 4;
constexpr int kTab1Bytes = kE * (kE - 1) * 8;      // the pass-1 twiddle table behind the image
constexpr int kCuLdsBytes = 160 * 1024;
constexpr int kRebias = 16;                        // 1 -> 2: outputs i' >= this take a second M0
// slot -> dword address
NW_SHAPE_HD constexpr int addr01(int i) { return (i % kE) * kS1 + i / kE; }
NW_SHAPE_HD constexpr int addr12(int i) { return ((i % 1024) / 32) * kS2 + (i / 1024) * 32 + i % 32; }
// writers: M0 (bytes from the image's start) of a wave, and the instruction's offset field
NW_SHAPE_HD constexpr int m0_01(int wave) { return 256 * wave; }
NW_SHAPE_HD constexpr int off_01(int p) { return 4 * p * kS1; }
NW_SHAPE_HD constexpr int m0_12(int wave, int ip) { return 256 * wave + (ip >= kRebias ? 4 * kRebias * kS2 : 0); }
NW_SHAPE_HD constexpr int off_12(int ip) { return 4 * (ip % kRebias) * kS2; }
// readers: one base per lane (dwords) plus a compile-time offset per element r
NW_SHAPE_HD constexpr int rbase_01(int u) { return (u % kE) * kS1 + u / kE; }
NW_SHAPE_HD constexpr int roff_01(int r) { return (kT / kE) * r; }
NW_SHAPE_HD constexpr int rbase_12(int j2) { return (j2 / 32) * kS2 + j2 % 32; }
NW_SHAPE_HD constexpr int roff_12(int r) { return 32 * r; }
static_assert(addr01(kN - 1) < kElems && addr12(kN - 1) < kElems, "both images inside the region");
static_assert(off_01(kE - 1) < 65536 && off_12(kE - 1) < 65536, "16-bit offset field");
static_assert(2 * (kBytes + kTab1Bytes) <= kCuLdsBytes, "two blocks per CU");

// 8-byte LDS reads of these kernels issued one ds_read_b64 each from inline asm (nw_fft_dev.h,
// ds_read_b64_*): left to the compiler, neighbouring reads are merged into ds_read2_b64 /
// ds_read2st64_b64, which take twice the LDS cycles of the two reads they replace.
// NW_LDS_ASM_READS is a mask of the sites: 1 the 1 -> 2 image's paired reads, 2 the pass-1
// twiddle table.  0: the compiler's loads.  (A third site, the pass-0 X image that the LDS-DMA
// fills, measured -0.5 % per launch at best and is not built: DESIGN.md §4 Round 15.)
#ifndef NW_LDS_ASM_READS
#define NW_LDS_ASM_READS 3
#endif
constexpr int kAsmReadImage = 1, kAsmReadTab1 = 2;
// Every read is (one byte base per lane) + (a compile-time byte offset, the instruction's
// unsigned 16-bit field); bases count from the start of the block's LDS.
// 1 -> 2 image: thread t reads the pairs (2t, 2t + 1) of elements r < 16
NW_SHAPE_HD constexpr int rd12_base(int t) { return 4 * rbase_12(2 * t); }
NW_SHAPE_HD constexpr int rd12_off(int r) { return 4 * roff_12(r); }
// pass-1 table (behind the image; power r = 1 .. 31 of column jj at entry (r - 1) * 32 + jj, 8 B
// each): butterfly t reads column t % 32, in batches b = 0 .. 3 of the pairs (w^r, w^(r + 16)),
// r = 4 b .. 4 b + 3 (w^0 is not stored: batch 0 has 7 entries)
constexpr int kTabBatch = 4;
NW_SHAPE_HD constexpr int tab1_base(int t) { return kBytes + 8 * (t % kE); }
NW_SHAPE_HD constexpr int tab1_off(int r) { return 8 * kE * (r - 1); }
static_assert(rd12_off(15) < 65536 && tab1_off(kE - 1) < 65536, "16-bit offset field");
}  // namespace lane_image

// ---- multi-channel connectivity (nw_conn.hip) -------------------------------------------------

// nw_conn_accumulate_kernel: a block owns one scale, kConnTileN consecutive output samples (lane =
// sample) and one pair tile: at most kConnPairs pairs that together touch at most kConnCh distinct
// channels (the host tiler nw::host::conn_tiles).  Its kConnWaves waves split the tile's pairs
// (wave w: pairs w, w + kConnWaves, ...), so a wave keeps kConnPairs / kConnWaves complex fp64
// accumulators in registers; per epoch the tile's channels are staged once in LDS as fp64.
constexpr int kConnPairs = 64;
constexpr int kConnCh = 16;
constexpr int kConnTileN = 64;
constexpr int kConnWaves = 4;
constexpr int kConnPerWave = kConnPairs / kConnWaves;
static_assert(kConnPairs % kConnWaves == 0 && kConnCh % kConnWaves == 0, "conn geometry");
// One pair tile as the kernel reads it: the channels it stages, and per pair the two staging slots
// (indices into ch[]) and the row of the caller's pair list the sums belong to.
struct ConnTile {
    int32_t nch, npairs;
    int32_t ch[kConnCh];
    int32_t sa[kConnPairs], sb[kConnPairs], out[kConnPairs];
};
// block -> (unit, pair tile), a unit being one (scale, sample tile).  xcd = true: blocks b, b + 8,
// ... share an XCD, and the pair tiles of one unit are consecutive among them, so the unit's rows
// are read from HBM once and then from that XCD's L2; units are padded to a multiple of 8 (a slot
// with unit >= nunits is padding and its block returns).  xcd = false: pair tile fastest in plain
// block order (consecutive blocks go to consecutive XCDs).
struct ConnSlot {
    int64_t unit;
    int tile;
};
NW_SHAPE_HD NW_INLINE ConnSlot conn_slot(int64_t b, int ntiles, bool xcd) {
    if (!xcd) return {b / ntiles, (int)(b % ntiles)};
    const int64_t local = b >> 3;
    return {(local / ntiles) * 8 + (b & 7), (int)(local % ntiles)};
}
constexpr int64_t conn_units(int nfreq, int64_t n_out) { return (int64_t)nfreq * ((n_out + kConnTileN - 1) / kConnTileN); }
constexpr int64_t conn_blocks(int64_t nunits, int ntiles, bool xcd) {
    return (xcd ? (nunits + 7) / 8 * 8 : nunits) * ntiles;
}

// ---- over-time connectivity (nw_conn_time.hip) ------------------------------------------------

// nw_conn_time_kernel: a block owns one epoch e of the chunk, one scale f and one pair tile, and
// sums over the window's samples s_j = t0 + j * step, j = 0 .. T - 1.  Its unit is e * F + f; the
// block order is conn_slot's (the pair tiles of one (e, f) neighbours on one XCD).
struct ConnTimeSlot {
    int64_t e;   // epoch of the chunk; >= ec: padding of the XCD order
    int f, tile;
};
NW_SHAPE_HD NW_INLINE ConnTimeSlot conn_time_slot(int64_t b, int nfreq, int ntiles, bool xcd) {
    const ConnSlot sl = conn_slot(b, ntiles, xcd);
    return {sl.unit / nfreq, (int)(sl.unit % nfreq), sl.tile};
}
constexpr int64_t conn_time_blocks(int64_t ec, int nfreq, int ntiles, bool xcd) {
    return conn_blocks(ec * nfreq, ntiles, xcd);
}
// T: the samples t0, t0 + step, ... < t1 (0 <= t0 <= t1, step >= 1)
constexpr int64_t conn_time_count(int64_t t0, int64_t t1, int64_t step) { return (t1 - t0 + step - 1) / step; }
// The summation order (the contract of nw_execute_conn_time, ninwave.h): lane conn_time_lane(j)
// adds the terms of its samples j in increasing order to an accumulator that starts at +0.0; the
// kConnTileN lane values are then folded, v_l <- v_l + v_{l xor d} for d = 32, 16, 8, 4, 2, 1,
// and lane 0 holds the sum.
constexpr int conn_time_lane(int64_t j) { return (int)(j % kConnTileN); }
constexpr int64_t conn_time_tiles(int64_t count) { return (count + kConnTileN - 1) / kConnTileN; }
static_assert(conn_time_count(0, 0, 1) == 0 && conn_time_count(37, 1001, 1) == 964 && conn_time_count(0, 1, 4) == 1 &&
                  conn_time_count(8, 1000, 4) == 248 && conn_time_count(8, 1001, 4) == 249,
              "window sample count");
static_assert(conn_time_lane(0) == 0 && conn_time_lane(63) == 63 && conn_time_lane(64) == 0 && conn_time_tiles(65) == 2,
              "lane of a sample");
static_assert(conn_time_blocks(2, 9, 3, false) == 54 && conn_time_blocks(2, 9, 3, true) == 72, "block count");

// ---- phase-amplitude coupling (nw_pac.hip) ----------------------------------------------------

// nw_pac_kernel: a block owns one epoch e of the chunk, one channel pair and one scale tile of at
// most kPacPh listed phase scales x kPacAm listed amplitude scales; wave w of its kPacWaves keeps the
// amplitude scales w * kPacAmWave .. of the tile against all kPacPh phase scales in registers
// (kPacAmWave * kPacPh complex fp64 accumulators), lane = sample of a kConnTileN-sample tile, and the
// sums run in conn_time_lane's order.  Per sample tile every wave stages kPacStagePh phase rows (as
// unit phasors) and kPacStageAm amplitude rows (as magnitudes) in LDS.
constexpr int kPacPh = 8;
constexpr int kPacAm = 16;
constexpr int kPacWaves = 4;
constexpr int kPacAmWave = kPacAm / kPacWaves;
constexpr int kPacStagePh = kPacPh / kPacWaves;
constexpr int kPacStageAm = kPacAm / kPacWaves;
static_assert(kPacAm % kPacWaves == 0 && kPacPh % kPacWaves == 0, "pac geometry");
static_assert(2 * (2 * kPacPh + kPacAm) * kConnTileN * 8 <= 64 * 1024, "double-buffered staging fits the LDS of a block");
constexpr int64_t pac_tiles_ph(int64_t nph) { return (nph + kPacPh - 1) / kPacPh; }
constexpr int64_t pac_tiles_am(int64_t nam) { return (nam + kPacAm - 1) / kPacAm; }
// The scale tiles of one (epoch, pair), amplitude tile fastest (pac_blocks is -1 where their count does
// not fit conn_slot's 32-bit tile index).
constexpr int64_t pac_tiles(int64_t nph, int64_t nam) { return pac_tiles_ph(nph) * pac_tiles_am(nam); }
// block -> (epoch, pair, phase tile, amplitude tile).  The unit of conn_slot is e * npairs + pair: in the
// XCD order the scale tiles of one (epoch, pair) -- which read the same two channels' rows -- are
// neighbours on one XCD, and the units are padded to a multiple of 8 (a slot with e >= ec is padding
// and its block returns).  ntiles = pac_tiles(nph, nam) >= 1, nta = pac_tiles_am(nam), npairs >= 1.
struct PacSlot {
    int64_t e;   // epoch of the chunk; >= ec: padding of the XCD order
    int pair, tp, ta;
};
NW_SHAPE_HD NW_INLINE PacSlot pac_slot(int64_t b, int npairs, int ntiles, int nta, bool xcd) {
    const ConnSlot sl = conn_slot(b, ntiles, xcd);
    return {sl.unit / npairs, (int)(sl.unit % npairs), sl.tile / nta, sl.tile % nta};
}
constexpr int64_t pac_blocks(int64_t ec, int64_t npairs, int64_t ntiles, bool xcd) {
    return ntiles > 0x7fffffff ? -1 : conn_blocks(ec * npairs, (int)ntiles, xcd);
}
static_assert(pac_tiles_ph(8) == 1 && pac_tiles_ph(9) == 2 && pac_tiles_am(16) == 1 && pac_tiles_am(17) == 2 &&
                  pac_tiles(9, 17) == 4 && pac_tiles(0, 5) == 0,
              "scale tile counts");
static_assert(pac_blocks(2, 5, 4, false) == 40 && pac_blocks(2, 5, 4, true) == 64 && pac_blocks(0, 5, 4, true) == 0,
              "block count");

// ---- time-lag surrogates of the phase-amplitude coupling (nw_pac_surr.hip) ---------------------

// nw_pac_stage_kernel leaves, per chunk and in WINDOW order (index j = 0 .. T - 1: t0 and step drop out), the
// unit phasors of every signal's listed phase scales as two planes and the magnitudes of its listed
// amplitude scales, in fp64; a thread owns one (row, j), kPacSurrStageThreads consecutive j per block:
//   [pac_surr_phase_at(sig, i, comp, nph, T) + j]        comp 0: re, 1: im       2 nsig nph T doubles, then
//   [pac_surr_amp_at(nsig, sig, k, nph, nam, T) + j]                              nsig nam T doubles
// nw_pac_surr_kernel: nw_pac_kernel's block map, tile and wave split on those values; for the lag l the
// amplitude sample of the term j is pac_surr_wrap(j, l, T) (l in [0, T): one conditional subtract, no %),
// and after each lag's fold lane pac_surr_cell_lane(k, q) of a wave keeps the cell (amplitude slot k of the
// wave, phase slot q)'s statistics.
constexpr int kPacSurrStageThreads = 256;
constexpr int64_t pac_surr_stage_doubles(int64_t nsig, int64_t nph, int64_t nam, int64_t T) {
    return nsig * (2 * nph + nam) * T;
}
constexpr int64_t pac_surr_phase_at(int64_t sig, int64_t i, int comp, int64_t nph, int64_t T) {
    return ((sig * nph + i) * 2 + comp) * T;
}
constexpr int64_t pac_surr_amp_at(int64_t nsig, int64_t sig, int64_t k, int64_t nph, int64_t nam, int64_t T) {
    return nsig * 2 * nph * T + (sig * nam + k) * T;
}
// the blocks of the staging launch: nrows = nsig (nph + nam) rows of T samples
constexpr int64_t pac_surr_stage_tiles(int64_t T) { return (T + kPacSurrStageThreads - 1) / kPacSurrStageThreads; }
constexpr int64_t pac_surr_stage_blocks(int64_t nrows, int64_t T) { return nrows * pac_surr_stage_tiles(T); }
constexpr int64_t pac_surr_wrap(int64_t j, int64_t l, int64_t T) { return j + l >= T ? j + l - T : j + l; }
constexpr int pac_surr_cell_lane(int k, int q) { return k * kPacPh + q; }
static_assert(kPacAmWave * kPacPh <= 64, "a wave's cells: one lane each");
static_assert(pac_surr_stage_doubles(6, 4, 5, 964) == 6 * 13 * 964 &&
                  pac_surr_amp_at(6, 0, 0, 4, 5, 964) == pac_surr_phase_at(6, 0, 0, 4, 964) &&
                  pac_surr_amp_at(6, 5, 4, 4, 5, 964) + 964 == pac_surr_stage_doubles(6, 4, 5, 964),
              "the staged planes tile the scratch");
static_assert(pac_surr_stage_tiles(0) == 0 && pac_surr_stage_tiles(256) == 1 && pac_surr_stage_tiles(257) == 2 &&
                  pac_surr_stage_blocks(78, 964) == 312,
              "staging blocks");
static_assert(pac_surr_wrap(0, 0, 5) == 0 && pac_surr_wrap(4, 4, 5) == 3 && pac_surr_wrap(1, 4, 5) == 0 &&
                  pac_surr_wrap(0, 4, 5) == 4 && pac_surr_wrap(0, 0, 1) == 0,
              "the circular shift");
static_assert(pac_surr_cell_lane(0, 0) == 0 && pac_surr_cell_lane(kPacAmWave - 1, kPacPh - 1) == kPacAmWave * kPacPh - 1,
              "cell lanes");

// ---- event-related phase-amplitude coupling (nw_erpac.hip) -------------------------------------

// nw_erpac_kernel: nw_pac_kernel's scale tile and wave split with the sum taken over the EPOCHS of the
// chunk: a block owns one channel pair, one sample tile of kConnTileN consecutive window samples (lane =
// sample) and one scale tile; its kPacAmWave * kPacPh complex fp64 accumulators per lane are loaded from
// the call's sums at the start of a launch and stored back at its end.
constexpr int64_t erpac_sample_tiles(int64_t count) { return conn_time_tiles(count); }
// block -> (pair, sample tile, phase tile, amplitude tile).  The unit of conn_slot is pair * nst + st: in
// the XCD order the scale tiles of one (pair, sample tile) -- which read the same samples of the same two
// channels' rows -- are neighbours on one XCD, and the units are padded to a multiple of 8 (a slot with
// pair >= npairs is padding and its block returns).  nst = erpac_sample_tiles(T) >= 1, ntiles =
// pac_tiles(nph, nam) >= 1, nta = pac_tiles_am(nam).
struct ErpacSlot {
    int64_t pair;   // >= npairs: padding of the XCD order
    int64_t st;
    int tp, ta;
};
NW_SHAPE_HD NW_INLINE ErpacSlot erpac_slot(int64_t b, int64_t nst, int ntiles, int nta, bool xcd) {
    const ConnSlot sl = conn_slot(b, ntiles, xcd);
    return {sl.unit / nst, sl.unit % nst, sl.tile / nta, sl.tile % nta};
}
// (-1 where the scale tiles do not fit conn_slot's 32-bit tile index; 0 for an empty window)
constexpr int64_t erpac_blocks(int64_t npairs, int64_t nst, int64_t ntiles, bool xcd) {
    return ntiles > 0x7fffffff ? -1 : conn_blocks(npairs * nst, (int)ntiles, xcd);
}
static_assert(erpac_sample_tiles(0) == 0 && erpac_sample_tiles(64) == 1 && erpac_sample_tiles(65) == 2 &&
                  erpac_sample_tiles(1201) == 19,
              "sample tile count");
static_assert(erpac_blocks(5, 19, 4, false) == 380 && erpac_blocks(5, 19, 4, true) == 384 && erpac_blocks(5, 0, 4, true) == 0 &&
                  erpac_blocks(0, 19, 4, true) == 0,
              "block count");

// ---- phase-binned phase-amplitude coupling (nw_pac_bins.hip) -----------------------------------

// nw_pac_bins_kernel: a block owns one epoch e of the chunk, one channel pair, ONE listed phase scale
// and a tile of kPacBinsWaves * ka listed amplitude scales; wave w keeps the tile's amplitude scales
// w * ka .. w * ka + ka - 1, lane = sample of a kConnTileN-sample tile, sums in conn_time_lane's order.
// A lane's nbins * ka partial sums are addressed by a run-time bin, so they live in LDS and not in
// registers: acc[w][bin * ka + k][lane] in fp64, a wave's accesses differing in the lane term only
// (conflict-free), cap * ka * 512 B per wave with cap >= nbins the bins the build holds.  The geometry is
// chosen from nbins so that two blocks fit a CU's 160 KiB: fewer bins, more amplitude scales per wave.
constexpr int kPacBinsWaves = 4;
constexpr int kPacBinsMax = NW_PAC_MAX_BINS;
static_assert(kPacBinsMax == 36, "the geometry classes below");
struct PacBinsGeom {
    int cap, ka;   // bins the accumulators hold, amplitude scales per wave
};
constexpr PacBinsGeom pac_bins_geom(int nbins) {
    return nbins <= 8 ? PacBinsGeom{8, 4} : nbins <= 18 ? PacBinsGeom{18, 2} : PacBinsGeom{kPacBinsMax, 1};
}
constexpr bool pac_bins_valid(int64_t nbins) { return nbins >= 2 && nbins <= kPacBinsMax && nbins % 2 == 0; }
// the amplitude scales of a tile, and the static LDS of a block: the accumulators, the double-buffered
// bin indices of kPacBinsWaves sample tiles and the edge table
constexpr int pac_bins_am(int nbins) { return kPacBinsWaves * pac_bins_geom(nbins).ka; }
constexpr int64_t pac_bins_lds(int nbins) {
    return (int64_t)kPacBinsWaves * pac_bins_geom(nbins).cap * pac_bins_geom(nbins).ka * kConnTileN * 8 +
           2 * kPacBinsWaves * kConnTileN * 4 + pac_bins_geom(nbins).cap * 16;
}
constexpr int64_t pac_bins_tiles_am(int64_t nam, int nbins) { return (nam + pac_bins_am(nbins) - 1) / pac_bins_am(nbins); }
// The tiles of one (epoch, pair): listed phase scale x amplitude tile, amplitude tile fastest.  block ->
// (epoch, pair, phase position, amplitude tile) is pac_slot(b, npairs, ntiles, nta, xcd) with tp the phase
// position, and the grid is pac_blocks(ec, npairs, ntiles, xcd).
constexpr int64_t pac_bins_tiles(int64_t nph, int64_t nam, int nbins) { return nph * pac_bins_tiles_am(nam, nbins); }
static_assert(pac_bins_geom(2).ka == 4 && pac_bins_geom(8).ka == 4 && pac_bins_geom(10).ka == 2 &&
                  pac_bins_geom(18).ka == 2 && pac_bins_geom(20).ka == 1 && pac_bins_geom(36).cap == 36,
              "geometry classes");
static_assert(2 * pac_bins_lds(2) <= 160 * 1024 && 2 * pac_bins_lds(18) <= 160 * 1024 && 2 * pac_bins_lds(36) <= 160 * 1024,
              "two blocks per CU");
static_assert(pac_bins_tiles(9, 17, 18) == 27 && pac_bins_tiles(9, 17, 36) == 45 && pac_bins_tiles(9, 17, 4) == 18 &&
                  pac_bins_tiles(0, 5, 18) == 0,
              "tile counts");

// ---- the two-pass engine (nw_large.hip) -----------------------------------------------------

// power-of-two 2^15 <= n <= 2^24, fp32 or fp64
constexpr int kLargeLog2Min = 15, kLargeLog2Max = 24;
constexpr bool large_supported(int64_t n, int dtype) {
    return (dtype == NW_F32 || dtype == NW_F64) && n >= (int64_t(1) << kLargeLog2Min) &&
           n <= (int64_t(1) << kLargeLog2Max) && !(n & (n - 1));
}

// rows of at most 16384 on chip, fp64 too (N2 = 8192 with N1 = 2048, 8-column blocks and
// 128-B runs: C5 fp64 150.0 ms/step; 16384, 16 columns, 256-B runs: 129.9)
// (fp32 rows of 32768 -- N1 = 512, 64-column workgroups writing 512-B output pieces -- measured
// in round 6: the row pass at one 1024-thread block per CU +37-43 %, the column pass 0-3 %
// faster, C5 step +10 %; profiles/r06_c5_rows32k_ab.txt)
constexpr int kMaxN2 = 16384;
// n = N1 * N2: N2 = min(n / 32, 16384) in both dtypes (kMaxN2), N1 = n / N2 >= 32
struct Split {
    int n1, n2;
};
constexpr Split large_split(int64_t n) {
    const int64_t n1 = n / kMaxN2 > 32 ? n / kMaxN2 : 32;
    return {(int)n1, (int)(n / n1)};
}

// One visitor over the splits: f(LargeSplit<T, N1, N2>{}) for (n, dtype), `miss` past them.
template <typename T, int N1, int N2> struct LargeSplit {};
template <typename T, int LG, typename R, typename F>
inline R for_large_length(int64_t n, R miss, F& f) {
    if constexpr (LG > kLargeLog2Max) {
        return miss;
    } else {
        constexpr Split sp = large_split(int64_t(1) << LG);
        if (n == (int64_t(1) << LG)) return f(LargeSplit<T, sp.n1, sp.n2>{});
        return for_large_length<T, LG + 1>(n, miss, f);
    }
}
template <typename R, typename F>
inline R for_large_split(int64_t n, int dtype, R miss, F f) {
    if (dtype == NW_F32) return for_large_length<float, kLargeLog2Min>(n, miss, f);
    if (dtype == NW_F64) return for_large_length<double, kLargeLog2Min>(n, miss, f);
    return miss;
}

// N2 (on-chip rows) and its elements per thread E, both dtypes: 32 from N2 = 8192 up, 16 below
template <typename T, int N2> constexpr int kRowE = N2 >= 8192 ? 32 : 16;
// complex table rows (wavelet_bin loads) spill at fp64 E = 32: E = 16 there
template <typename T, int N2> constexpr int kRowETab = sizeof(T) == 8 ? 16 : kRowE<T, N2>;
// rows (k1) per rows_kernel workgroup (XCD tile kRowTileF x kRowTileG above) ...
constexpr int kRowGroup = 4;
// ... of a launch over nf scales: 1 when it holds few scales (one row per block, more blocks)
constexpr int row_group_of(int nf) { return nf < kRowTileF ? 1 : kRowGroup; }
// Thread t of a row's N2 / E threads owns the bins k = k1 + n1 * (t + r * threads), r < E: with
// km the scale's last bin in the support, elements r >= row_need are zero for every thread
NW_SHAPE_HD constexpr NW_INLINE int row_need(int km, int k1, int n1, int threads) {
    return km < k1 ? 1 : (km - k1) / n1 / threads + 1;
}
// pass-0 variants of a row in steps of 4 elements at fp32 E = 32 (fp64: 4, 8, 16, 24, E): the
// row runs pass0_variant<E, kRowFine, (E > 16)>(row_need); table rows: more scratch
template <typename T, int E, bool TABLE> constexpr bool kRowFine = E > 16 && sizeof(T) == 4 && !TABLE;
// fp32 E = 32 rows: pruned Xt rows by LDS-DMA ahead of the stores (C5 50.6 -> 48.5 ms per step);
// analytic kinds only (table rows' wavelet_bin loads would exceed 128 VGPRs, as in nw_fused);
// fp64 rows with the same DMA measured no faster (0.94 -> 0.98 ms per launch; round 5, after the
// W-evaluator changes: rows -0.5 %, step +1.4 %, profiles/r05_c5f64_rows_xd_ab.txt)
// (fp64 rows with the DMA, re-measured in round 4 beside the fast Morse form: no gain either,
// profiles/r04_c5f64_rows_ab.txt)
template <typename T, int E, bool TABLE> constexpr bool kRowXD = sizeof(T) == 4 && E >= 32 && !TABLE;
// ... for a row whose pass 0 reads only Xt[k1][0 .. N2/2): variants NZ <= kRowLdsNz
template <int E> constexpr int kRowLdsNz = E / 2;

// cols_kernel workgroups of 1024 threads: C = 32 columns at N1 = 1024, 256-B runs (C5 cols
// 1.039 -> 0.978 ms per launch against 512 threads)
// cols_kernel workgroup size (C * N1 / E)
// fp64: 512 threads x 32 elements (N1 = 1024 in 2 passes, one exchange; 16 columns, 256-B runs
// as before) against 1024 x 16 (3 passes, two exchanges): C5 fp64 cols 3.97-4.11 -> 3.90-3.91
// ms per 32-scale launch (profiles/r05_c5f64_cols_e32_ab.txt; -DNW_COLS64_E16: the old form)
#ifdef NW_COLS64_E16
template <typename T> constexpr int kColThreads = 1024;
#else
template <typename T> constexpr int kColThreads = sizeof(T) == 8 ? 512 : 1024;
#endif
// elements per thread in cols_kernel: 32 complex fp32 (64 VGPRs) or fp64 (128 VGPRs, 2 waves/SIMD)
#ifdef NW_COLS64_E16
template <typename T> constexpr int kColE = sizeof(T) == 4 ? 32 : 16;
#else
template <typename T> constexpr int kColE = 32;
#endif
// fp32: the column-pair form (C5 cols 4.02 -> 3.86 ms per 64-scale launch against the
// single-column form, which fp64 keeps: its lanes already read and write 16 B;
// -DNW_COLS32_SINGLE: fp32 on the single-column form, diagnostic A/B)
#ifdef NW_COLS32_SINGLE
template <typename T> constexpr bool kColPair = false;
#else
template <typename T> constexpr bool kColPair = sizeof(T) == 4;
#endif
// The column pass's block: a thread owns one slot (CPS adjacent columns n2, one lane value) and
// E of a column's N1 points; a workgroup transforms C consecutive columns.  PAIR (fp32): two
// columns per slot at E = 16 -- length-N1 transforms at E = 16 take one exchange more than
// E = 32.  (E = 32 with 512-thread workgroups: one exchange instead of two, 198 VGPRs at
// 2 waves/SIMD: C5 cols 3.92 -> 3.95 ms per launch, not kept; profiles/r04_c5_colpairs_ab.txt)
template <typename T, bool PAIR, int N1> struct ColShape {
    static constexpr int E = PAIR ? 16 : kColE<T>;
    static constexpr int THREADS = PAIR ? 1024 : kColThreads<T>;
    static constexpr int U = N1 / E;                 // threads per slot
    static constexpr int SLOTS = THREADS / U;        // slots per workgroup
    static constexpr int CPS = PAIR ? 2 : 1;         // columns per slot
    static constexpr int C = SLOTS * CPS;            // columns per workgroup
    static constexpr int LDS = N1 * C * (int)sizeof(T);   // one real component of every point
    static_assert(N1 >= 32 && SLOTS >= (sizeof(T) == 4 ? 16 : 4), "cols geometry");
};

// bytes of B per launch pair (scales chunked to fit): 8 GiB = 64 scales of fp32 / 32 of fp64 at
// C5.  Against 2 GiB (16 / 8 scales): C5 fp32 47.49 -> 46.15 ms per step, fp64 118.19 -> 113.15
// (fewer, longer launches: the row pass's XCD tiles of 8 scales fill, fewer tails;
// profiles/r04_c5_fchunk.txt)
constexpr size_t kBBudget = size_t(8) << 30;
constexpr size_t large_cplx_bytes(int dtype) { return dtype == NW_F32 ? 8 : 16; }
// scales per launch pair: fc of them (at least one, at most all), by default what the budget holds
constexpr int64_t fchunk_clamp(int64_t fc, int nfreq) { return fc < 1 ? 1 : fc < nfreq ? fc : nfreq; }
constexpr int64_t fchunk_of(int64_t n, int nfreq, int dtype) {
    return fchunk_clamp((int64_t)(kBBudget / ((size_t)n * large_cplx_bytes(dtype))), nfreq);
}

// fp64 pass-0 twiddles w_n^m (m = n2 k1 < n) as the product of two exact entries:
// tsplit[m & 4095] = w_n^(m mod 4096) and tsplit[4096 + (m >> 12)] = w_n^(4096 (m >> 12))
constexpr int kSplitLo = 4096;
constexpr int kSplitEntries = 2 * kSplitLo;   // n <= 2^24: m >> 12 < 4096
// support buffer: kmax (int, padded to 256 B) | row maxima (u64) | tsplit (complex fp64)
constexpr size_t wmax_offset(int nfreq) { return ((size_t)nfreq * sizeof(int) + 255) / 256 * 256; }
constexpr size_t tsplit_offset(int nfreq) {
    return wmax_offset(nfreq) + ((size_t)nfreq * sizeof(uint64_t) + 255) / 256 * 256;
}
constexpr size_t large_support_bytes(int nfreq) { return tsplit_offset(nfreq) + kSplitEntries * 2 * sizeof(double); }

// ---- the chirp-z engine (nw_chirp.hip) ------------------------------------------------------

// (dtype, M) -> E of the chirp engine: fp32 M <= 16384 (E = 32 at 16384), fp64 M <= 8192;
// 0: no such kernel.  M = 1024 << c, c < kChirpClasses
constexpr int kChirpClasses = 5;
constexpr int64_t chirp_mmax(int dtype) { return dtype == NW_F32 ? 16384 : 8192; }
constexpr int chirp_e(int64_t m, int dtype) {
    if (dtype != NW_F32 && dtype != NW_F64) return 0;
    if (m < 1024 || m > chirp_mmax(dtype) || (m & (m - 1))) return 0;
    return m == 16384 ? 32 : 16;
}
// fp32 M = 8192: |y| and |y|^2 at E = 32 (256 threads, two blocks per CU, 3 passes, no
// scratch): measured N = 4097 power 10.60 -> 8.75 ms, N = 3001 6.60 -> 5.82 ms per launch;
// the complex output spills at E = 32 (108-128 B) and keeps E = 16
template <typename T, int M, int E> constexpr int kChirpAbsE = (sizeof(T) == 4 && M == 8192) ? 32 : E;

// One visitor over the table: f(ChirpSize<T, M, E>{}) for the row of (m, dtype), `miss` past it.
template <typename T, int M, int E> struct ChirpSize {};
template <typename T, int C, typename R, typename F>
inline R for_chirp_class(int64_t m, R miss, F& f) {
    if constexpr (C >= kChirpClasses || chirp_e(1024 << C, kDtypeOf<T>) == 0) {
        return miss;
    } else {
        if (m == (1024 << C)) return f(ChirpSize<T, (1024 << C), chirp_e(1024 << C, kDtypeOf<T>)>{});
        return for_chirp_class<T, C + 1>(m, miss, f);
    }
}
template <typename R, typename F>
inline R for_chirp_size(int64_t m, int dtype, R miss, F f) {
    if (dtype == NW_F32) return for_chirp_class<float, 0>(m, miss, f);
    if (dtype == NW_F64) return for_chirp_class<double, 0>(m, miss, f);
    return miss;
}

// the full transform length of n: M = 2^ceil(log2(2n - 1)), at least 1024
constexpr int64_t chirp_m(int64_t n) {
    int64_t m = 1024;
    while (m < 2 * n - 1) m <<= 1;
    return m;
}
// any n with 2n - 1 <= M_max that the power-of-two kernels do not take
constexpr bool chirp_supported(int64_t n, int dtype) {
    if (n < 1 || fused_supported(n, dtype)) return false;
    return (dtype == NW_F32 || dtype == NW_F64) && 2 * n - 1 <= chirp_mmax(dtype);
}
// longer lengths (up to M_max - 1) fit when every row's support does (M >= n + K - 1)
constexpr bool chirp_possible(int64_t n, int dtype) {
    if (n < 1 || fused_supported(n, dtype) || (dtype != NW_F32 && dtype != NW_F64)) return false;
    return n < chirp_mmax(dtype);
}
// The M class c (M = 1024 << c) of a row of length n whose support is ksup bins: M >= n + K - 1
// wrap-free, >= 2K for the pruned first pass 0, >= 1024, <= the full 2^ceil(log2(2n - 1)) and
// M_max; -1: wider than the largest on-chip transform
constexpr int chirp_class(int64_t n, int64_t ksup, int dtype) {
    const int64_t mfull = chirp_m(n) < chirp_mmax(dtype) ? chirp_m(n) : chirp_mmax(dtype);
    const int64_t wrap = n + (ksup > 1 ? ksup : 1) - 1;
    const int64_t need = wrap > 2 * ksup ? wrap : 2 * ksup;
    if (need > mfull) return -1;
    int c = 0;
    while ((int64_t(1024) << c) < need) ++c;
    return c;
}
// Epoch partial sums on the chirp-z form: every M class of the wavelet needs a partial-sum
// kernel without scratch (tools/regs.py): fp32 M <= 8192 (E = 16), fp64 power every M, fp64
// phases M <= 2048 (44-60 B of scratch above)
constexpr bool chirp_psum_ok(int dtype, bool phase, const int64_t* counts) {
    for (int c = 0; c < kChirpClasses; ++c) {
        if (counts[c] == 0) continue;
        const int64_t m = int64_t(1024) << c;
        if (dtype == NW_F32 ? m > 8192 : (phase && m > 2048)) return false;
    }
    return true;
}
// The chunk of such a reduction that starts at signal s0 of nsig (chunks of at most max_batch >= 1
// signals).  The kernel sums a block's signals in order into one partial row and the rows are added
// in order, so for the sums not to depend on max_batch the blocks must be the groups
// kPsumGroup g .. kPsumGroup g + kPsumGroup - 1 of the whole call: a chunk is whole groups (the
// call's last one ragged) or, where max_batch is shorter than a group, lies inside one group,
// whose partial row the next chunk carries on (s0 % kPsumGroup != 0) and which is added once
// complete.  The one-pass partial sums take the same chunks (execute_reduce, nw_api.cpp): their
// kernels cannot carry a row on, so a chunk inside a group leaves its signals' terms and the host
// path adds them in the block's order.
constexpr int64_t chirp_psum_chunk(int64_t s0, int64_t nsig, int64_t max_batch) {
    const int64_t left = nsig - s0, in_group = s0 % kPsumGroup;
    if (in_group == 0 && left <= max_batch) return left;
    if (in_group == 0 && max_batch >= kPsumGroup) return max_batch / kPsumGroup * kPsumGroup;
    const int64_t to_end = kPsumGroup - in_group;
    const int64_t c = max_batch < to_end ? max_batch : to_end;
    return c < left ? c : left;
}
static_assert(chirp_psum_chunk(0, 11, 11) == 11 && chirp_psum_chunk(0, 30, 11) == 8 && chirp_psum_chunk(24, 30, 11) == 6 &&
                  chirp_psum_chunk(0, 11, 4) == 4 && chirp_psum_chunk(8, 11, 4) == 3 && chirp_psum_chunk(6, 19, 3) == 2 &&
                  chirp_psum_chunk(16, 17, 3) == 1,
              "chunks of the chirp-z partial sums");

}  // namespace nw
