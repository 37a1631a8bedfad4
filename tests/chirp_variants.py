"""Which kernel instantiation the chirp-z form (nw_chirp.hip: every n that is not a power of two
>= 1024, up to M_max - 1) runs for a row and which pass-0 variant the row takes, restated from
nw_shape.h and nw_chirp.hip for the tests that steer rows into every one of them
(tests/test_gpu_chirp_rows.py, tests/test_chirp_cpu.py).

A row of length n whose W support is K bins (K = last non-zero bin + 1, chirp_support_kernel)
runs at the smallest transform M = 1024 << c that is wrap-free for it (M >= n + K - 1) and keeps
the pruned first pass 0 (M >= 2K), at most min(2^ceil(log2(2n - 1)), M_max); thread t of its
M / E threads owns the bins t + r M / E, r < E, and pass 0 reads only the elements r < NZ."""
import numpy as np

CLASSES = [1024, 2048, 4096, 8192, 16384]


def chirp_mmax(dtype):
    """The largest on-chip transform (chirp_mmax)."""
    return 16384 if dtype == 'float32' else 8192


def chirp_m(n):
    """The full transform length of n: 2^ceil(log2(2n - 1)), at least 1024 (chirp_m)."""
    m = 1024
    while m < 2 * n - 1:
        m <<= 1
    return m


def one_pass(n):
    """The power-of-two lengths the one-pass kernels take (fused_supported)."""
    return 1024 <= n <= 16384 and n & (n - 1) == 0


def chirp_supported(n, dtype):
    """Every row of such a length fits: 2n - 1 <= M_max (chirp_supported)."""
    return n >= 1 and not one_pass(n) and 2 * n - 1 <= chirp_mmax(dtype)


def chirp_possible(n, dtype):
    """... and the tentative lengths up to M_max - 1, whose rows fit if narrow (chirp_possible)."""
    return n >= 1 and not one_pass(n) and n < chirp_mmax(dtype)


def chirp_class(n, ksup, dtype):
    """The transform length M of a row of support ``ksup`` at length n, or -1 where the row is
    wider than the largest on-chip transform (chirp_class, which returns log2(M / 1024))."""
    mfull = min(chirp_m(n), chirp_mmax(dtype))
    need = max(n + max(ksup, 1) - 1, 2 * ksup)
    if need > mfull:
        return -1
    m = 1024
    while m < need:
        m <<= 1
    return m


def chirp_e(m, dtype, out='cwt'):
    """Elements per thread of the kernel that writes ``out`` at (dtype, M); 0: no such kernel.
    chirp_e: 16, and 32 at M = 16384; kChirpAbsE: |y| and |y|^2 at fp32 M = 8192 run at 32.  The
    partial-sum kernels (out 'power_sum' / 'phase_sum') exist at E = 16 only (launch_m_e)."""
    if dtype not in ('float32', 'float64') or m not in CLASSES or m > chirp_mmax(dtype):
        return 0
    e = 32 if m == 16384 else 16
    if out in ('abs', 'power') and dtype == 'float32' and m == 8192:
        return 32
    if out in ('power_sum', 'phase_sum') and e != 16:
        return 0
    return e


def psum_ok(dtype, phase, classes):
    """Whether an epoch reduction of rows in the transform sizes ``classes`` runs as partial sums
    inside the kernel (chirp_psum_ok): fp32 M <= 8192, fp64 power every M, fp64 phases M <= 2048."""
    for m in classes:
        if (m > 8192) if dtype == 'float32' else (phase and m > 2048):
            return False
    return True


def pass0_nz(ksup, m, e):
    """The pass-0 variant NZ of a row: the smallest of {1, 2, 4, e / 2} >= ceil(ksup / (m / e)),
    the `pass0` dispatch of nw_chirp_kernel (nw_chirp.hip: nz <= 1, <= 2, <= 4, else E / 2)."""
    tt = m // e
    need = (ksup + tt - 1) // tt
    assert need <= e // 2, 'a class holds only rows with 2K <= M'
    return min(v for v in (1, 2, 4, e // 2) if v >= need)


def table_support(row):
    """K of a table row as the plan holds it: the last non-zero bin + 1, 0 for an all-zero row
    (chirp_support_kernel)."""
    nz = np.flatnonzero(np.asarray(row) != 0)
    return int(nz[-1]) + 1 if nz.size else 0


def shannon_row(delta, n):
    """The Shannon row on a grid of spacing ``delta`` and length n: 1 where j * delta <= 1.0
    (psi_f64, the grid filled as np.arange fills it: j * step)."""
    return np.where(np.arange(n) * float(delta) <= 1.0, 1.0, 0.0)


def shannon_support(delta, n):
    """K of that row: (the last j with j * delta <= 1.0) + 1, capped at n."""
    return table_support(shannon_row(delta, n))


def shannon_delta(k):
    """The grid spacing whose Shannon row is 1 on [0, k): (k - 1) * delta < 1 < k * delta."""
    return 1.0 / (k - 0.5)


# ---- the inputs tests/test_chirp_cpu.py and tests/test_gpu_chirp_rows.py share

# n = M / 2 + WRAP_DELTA: the length at which one bin of wrap shows (tests/test_chirp_cpu.py)
WRAP_DELTA = 200


def wrap_case(m):
    """(n, K) of the tight wrap at transform size M: K = M - n + 1 is the last support in class M."""
    n = m // 2 + WRAP_DELTA
    return n, m - n + 1


def noise(S, n, seed, dtype):
    """White noise in the compute dtype (the reference sees the same rounded values)."""
    return np.random.default_rng(seed).standard_normal((S, n)).astype(dtype)


def hard_rows(supports, length, seed):
    """(len(supports), length) complex128: row i is complex normal on [0, supports[i]) divided by
    sqrt(supports[i]), exactly zero from there on (make_rows of tests/test_gpu_table_rows.py)."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((len(supports), length), dtype=np.complex128)
    for i, k in enumerate(supports):
        if k:
            tab[i, :k] = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.sqrt(k)
    return tab
