"""Which kernels the two-pass form (nw_large.hip, n = 2^15 .. 2^24) runs for a plan and which
pass-0 variant (pruned idft_br<T, E, NZ>) each of its rows takes, restated from nw_large.hip
for the tests that steer rows into every variant (tests/test_gpu_large_variants.py).

n = N1 * N2 (split_of); a row pass workgroup owns rows k1 of one scale, thread t of its
T = N2 / E threads the bins k = k1 + N1 * (t + r T), r < E (rows_kernel).  With km the scale's
last bin above the tail threshold (Plan.row_support()), elements r >= need(km, k1) are zero for
every thread, and the row runs the smallest instantiated NZ >= need (nzv_of).

tol_f32 is the two-pass form's fp32 tolerance against the fp64 oracle (test_gpu_large.py, where it is derived)."""


def tol_f32(n):
    """max |out - ref| <= tol_f32(n) max |ref|: 1e-5 up to n = 2^16, 3e-5 above."""
    return 1e-5 if n <= (1 << 16) else 3e-5


def split(n):
    """(N1, N2) of split_of: rows of at most kMaxN2 = 16384 on chip in both dtypes, N1 >= 32."""
    n1 = max(n // 16384, 32)
    return n1, n // n1


def row_elems(n2, dtype, table):
    """E of the row kernel (kRowE / kRowETab): 32 from N2 = 8192 up, else 16; fp64 complex
    table rows always 16."""
    if table and dtype == 'float64':
        return 16
    return 32 if n2 >= 8192 else 16


def ladder(e, dtype, table):
    """The pass-0 variants NZ instantiated for (E, dtype, analytic or table rows): nzv_of and
    the dispatch below it (steps of 4 only for fp32 analytic rows at E = 32)."""
    if e <= 16:
        return {4, 8, 16}
    if dtype == 'float32' and not table:
        return {4, 8, 12, 16, 20, 24, 32}
    return {4, 8, 16, 24, 32}


def need(km, k1, n1, t):
    """need_of(k1): pass-0 elements of row k1 that reach the support's last bin km."""
    return 1 if km < k1 else (km - k1) // n1 // t + 1


def variant(nd, lad):
    """The smallest NZ of the ladder that covers ``nd`` elements."""
    return min(v for v in lad if v >= nd)


def row_group(nf):
    """Rows per workgroup of a row-pass launch over nf scales (launch_row_pass: kRowGroup = 4
    from kRowTileF = 8 scales up)."""
    return 1 if nf < 8 else 4


def from_lds(e, dtype, table, nz):
    """Whether a row of variant NZ reads its Xt row from the LDS image (kRowsXD kernels: fp32
    analytic rows at E = 32 DMA a row that needs at most E / 2 elements) or from global memory."""
    return dtype == 'float32' and e == 32 and not table and nz <= 16
