"""Which pass-0 variant (pruned idft_br<T, E, NZ>) of the one-pass fused kernels a W row runs,
restated from ninwavelets_amd/csrc/nw_shape.h for the tests that steer rows into every
instantiated variant (tests/test_gpu_dft_forms.py: analytic rows, tests/test_gpu_table_rows.py:
table rows).  tests/test_host_asan.py compares this restatement, line by line, with what the
header itself gives for every row of the size table (tests/asan/host_asan.cpp, mode `shapes`), and
decim_rule with the header's decim_supported.

A row's support ends at its last bin above kTailRel x the row's max |W| (nw_internal.h);
wsupport_kernel rounds the pass-0 elements reaching it to wnz, pass0_variant picks the smallest
instantiated NZ >= wnz.  (wsupport_kernel<T, false> measures a complex bin by max(|re|, |im|),
row_wnz by |w|: the two agree on rows whose support has a hard edge.)"""
import numpy as np

TAIL_REL = {'float64': 2.0 ** -72, 'float32': 2.0 ** -56}      # kTailRel (nw_internal.h)


def elems_per_thread(n):
    """E of the fused kernels (fused_e, nw_shape.h): 16 up to n = 4096, 32 above."""
    return 16 if n <= 4096 else 32


def instantiated_variants(n, dtype, out, pair):
    """The pass-0 variants NZ of the kernel that runs (n, dtype, out): pass0_variant
    (nw_shape.h) for the single-signal kernel, the pair kernel's own ladder (pair_pass0_variant)."""
    e = elems_per_thread(n)
    if pair:
        return {4, 8, 12, e}
    v = {4, 8, e}
    if e > 16:
        v |= {16, 24}
        if dtype == 'float32' or out == 'cwt':
            v |= {12, 20}
    return v


def row_wnz(row, n, dtype):
    """wnz of one W row as wsupport_kernel builds it: pass-0 elements reaching the support,
    rounded up (wnz_round, nw_shape.h) to 1, 2, 4, 8, then to a multiple of 4, capped at E."""
    e = elems_per_thread(n)
    mag = np.abs(np.asarray(row))
    mag = np.where(np.isfinite(mag), mag, 0.0)
    above = np.nonzero(mag > TAIL_REL[dtype] * mag.max())[0]
    need = 1 if above.size == 0 else int(above[-1]) // (n // e) + 1
    p2 = 1
    while p2 < need and p2 < 8:
        p2 *= 2
    if p2 < need:
        p2 = (need + 3) // 4 * 4
    return min(p2, e), need


def variant_of(wnz, variants):
    return min(v for v in variants if v >= max(wnz, 4))


def decim_rule(n, decim):
    """Where the decimated kernel runs (decim_supported, nw_shape.h): power-of-two 2048 <= n <= 16384, power-of-two
    decim >= 2, n / decim >= 1024."""
    pow2 = lambda v: v > 0 and v & (v - 1) == 0  # noqa: E731
    return pow2(n) and 2048 <= n <= 16384 and pow2(decim) and decim >= 2 and n // decim >= 1024
