"""GPU parity of the one-pass kernels with real W rows -- nw_fused_kernel<..., REALW = true>,
nw_fused_pair_kernel and fwd_r2c_kernel (nw_fused.hip) -- per row, with a hard-edged row at both
ends of every pruning bucket.  tests/test_gpu_dft_forms.py, test_gpu_lane_image.py and
test_gpu_lds_reads.py cover these kernels with narrowband signals under one maximum over all rows
and with soft-edged rows deep inside their buckets; here the signals have a flat spectrum, every
(signal, row) is held to a maximum it reaches itself, and the row's last bin is worth over 200
times the fp32 bound (tests/test_fused_cases_cpu.py asserts that, and the other conditions on the
inputs, on the reference alone).  Inputs: tests/fused_cases.py.

Reference: oracle.nw_oracle.cwt_from_rows in complex128 on the rows the plan holds (plan.rows();
tests/test_gpu_wavelet_rows.py holds the row evaluator to the oracle), |.| and |.|^2 taken from it,
the epoch sums formed from it in fp64 in signal order.  TOL is the contract of
tests/test_gpu_parity.py, 1e-12 (fp64) / 1e-5 (fp32), doubled for |y|^2.

  A. every (n, dtype, kind) x every K of fused_cases.supports(n): cwt, |y| and |y|^2 of S = 5
     signals in one chunk (the pair kernel: pairs (0, 1), (2, 3) and an odd last signal; the
     single-signal kernel: blocks of 2, 2 and 1), for every (signal, row)
         max|got - want| <= TOL x (2 if power) x max|want|  over that row alone;
     at K = 4 TT + 1 also the first signal and the first two alone, bit for bit the S = 5 result.
     The same at K = n / 2 + 1 and K = n with Nyquist bins of alternating sign (in A's signals the
     bin, which the kernels carry one signal ahead in registers, is the same in every signal).
  B. power_sum and phase_sum of the same plans at max_batch = 5 and at max_batch = 2: bit-identical;
     reduce_path as fused_cases.PARTIALS says (n = 8192 with fp32 phases or fp64 runs the E = 16
     partial-sum kernel on a support table built for E = 32);
         |d power_sum[k]| <= 2 TOL sum_s max|ref_s row|^2,
         |d phase_sum[k]| <= 2 TOL sum_s max|ref_s row| / |ref_s[k]|  where that is <= 0.05,
     the other phase points finite with modulus <= S + 1e-6.  At fp32 with n <= 4096 also
     cross_sum and plv_sum of the pairs (x0, x1), (x2, x3) at the K around kPairWKeepRed and the
     variant 12, with the same kind of bound from the two channels' row maxima.
  C. blocks of 8 signals of the single-signal output kernel: Morse on the ordinary grid, 256
     scales, 67 signals in one launch on device tensors; executing two signals of it alone (blocks
     of 2) gives the same bits at every position inside a block of 8, in two XCD slots and in the
     ragged last block; signals 3 and 66 at seven rows against oracle.nw_oracle.cwt at A's bound.

Measured on an MI355X, worst err / bound over both kinds and every K (the contract holds on
every row of the unmodified kernels with a factor 17 to spare, so no bound here was widened):
    A and B     n     cwt    |y|    |y|^2   power_sum  phase_sum
    fp32     1024    0.039  0.037  0.033      0.011      0.008
    fp32     2048    0.045  0.046  0.042      0.015      0.008
    fp32     4096    0.050  0.049  0.047      0.018      0.008
    fp32     8192    0.053  0.055  0.048      0.017      0.009
    fp32    16384    0.054  0.055  0.053      0.018      0.010
    fp64   every n  <= 0.001 for cwt, |y|, |y|^2; < 0.0005 for both sums
    A with alternating Nyquist bins: fp32 <= 0.051, fp64 <= 0.001; sums <= 0.015
    B pairs (fp32, n <= 4096): S_ab <= 0.013, P_aa and P_bb <= 0.023, plv <= 0.008
    C: fp32 8192 cwt 0.054, |y|^2 0.046; 16384 |y| 0.058, |y|^2 0.054; fp64 0.001
B's bit-identity found the one-pass partial sums regrouped by max_batch (fp64 power_sum and every
phase_sum differed in the last bits, <= 1.3e-15 absolute, at every K of every case with
NW_REDUCE_PARTIALS); execute_reduce (nw_api.cpp) now adds a short chunk's terms in the block's order.
"""
import numpy as np
import pytest

import fused_cases as C
from fused_variants import elems_per_thread
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

KINDS = sorted(C.KIND_PARAMS)
S = C.S


def make_plan(n, dtype, kind, k, max_batch):
    """F = 3 hard-edged rows of support [0, k)."""
    p = nw.Plan(n, len(C.PEAKS), dtype, max_batch=max_batch)
    try:
        p.set_wavelet(kind, C.KIND_PARAMS[kind], C.freqs_of(k), L.nw_grid(1.0, n, k))
    except Exception:
        p.close()
        raise
    return p


_refs = {}


def case_reference(p, n, dtype, kind, k, nyquist=None):
    """(x, ref (S, F, n) complex128) of a plan's own rows: computed once per case; a later plan of
    the case must hold the same rows, which end exactly at bin k - 1."""
    rows = p.rows()
    assert rows.shape == (len(C.PEAKS), n) and rows.dtype == np.dtype(dtype)
    assert np.all(rows[:, k:] == 0) and np.all(rows[:, k - 1] != 0), (kind, n, dtype, k)
    key = (n, dtype, kind, k, nyquist)
    x = C.signals(n, dtype, S, nyquist)
    if key not in _refs:
        _refs[key] = (rows, C.reference(x, rows))
    assert np.array_equal(rows, _refs[key][0])
    return x, _refs[key][1]


def kernel_name(n, dtype):
    return 'nw_fused_pair_kernel' if C.pair_kernel(n, dtype) else 'nw_fused_kernel'


def row_excess(got, want, dtype, out):
    """(S, F): each row's max|got - want| over its bound, tol x max|want| of that row."""
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.max(np.abs(got - want), axis=-1) / (C.tol_of(dtype, out) * np.max(np.abs(want), axis=-1))


# ------------------------------------------------------------------ A. every row, every edge
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', C.DTYPES)
@pytest.mark.parametrize('n', C.SIZES)
def test_every_row_at_every_support_edge(n, dtype, kind):
    tt = n // elems_per_thread(n)
    worst = {out: (0.0, None) for out in C.OUTS}
    for k in C.supports(n):
        p = make_plan(n, dtype, kind, k, S)
        try:
            x, ref = case_reference(p, n, dtype, kind, k)
            for out in C.OUTS:
                got = np.array(p.execute(x, out_kind=out))
                st = p.stats()
                assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == kernel_name(n, dtype), (k, out, st)
                e = float(np.max(row_excess(got, C.as_kind(ref, out), dtype, out)))
                if e > worst[out][0]:
                    worst[out] = (e, k)
                if k == 4 * tt + 1:
                    for cnt in (1, 2):
                        np.testing.assert_array_equal(np.array(p.execute(x[:cnt], out_kind=out)), got[:cnt])
        finally:
            p.close()
    for out in C.OUTS:
        print(f'A {kind} n={n} {dtype} {out}: worst err / bound {worst[out][0]:.3f} at K = {worst[out][1]}')
    assert all(e <= 1.0 for e, _ in worst.values()), worst


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', C.DTYPES)
@pytest.mark.parametrize('n', C.SIZES)
def test_nyquist_bin_of_every_signal(n, dtype, kind):
    """The signals of A share one Nyquist bin, which the kernels carry one signal (one pair) ahead
    in registers.  Here its sign alternates, so the second signal of every block of 2 differs from
    the first in it, at K = n / 2 + 1 (the Nyquist bin is the row's last) and K = n: a stale bin
    is twice the last bin's worth, over 400 times the fp32 bound.  Outputs at A's bound, the epoch
    sums (blocks of 5) at B's."""
    worst = {out: 0.0 for out in C.OUTS + ['power_sum', 'phase_sum']}
    for k in (n // 2 + 1, n):
        p = make_plan(n, dtype, kind, k, S)
        try:
            x, ref = case_reference(p, n, dtype, kind, k, C.NYQUIST_ALTERNATE)
            for out in C.OUTS:
                got = np.array(p.execute(x, out_kind=out))
                worst[out] = max(worst[out], float(np.max(row_excess(got, C.as_kind(ref, out), dtype, out))))
            res = {out: np.array(p.execute(x, out_kind=out)) for out in ('power_sum', 'phase_sum')}
        finally:
            p.close()
        for out, e in zip(('power_sum', 'phase_sum'), epoch_excess(res, ref, dtype)):
            worst[out] = max(worst[out], e)
    print(f'A nyquist {kind} n={n} {dtype}: worst err / bound ' + ', '.join(f'{o} {e:.3f}' for o, e in worst.items()))
    assert all(e <= 1.0 for e in worst.values()), worst


# ------------------------------------------------------------------ B. partial sums at the same edges
def epoch_excess(res, ref, dtype):
    """Worst err / bound of power_sum and of phase_sum at the points under the cap; the other
    phase points finite with modulus <= S + 1e-6."""
    ps, ph = C.epoch_sums(ref)
    e_ps = float(np.max(np.abs(res['power_sum'] - ps) / C.power_sum_bound(ref, dtype)))
    bound = C.phase_sum_bound(ref, dtype)
    good = bound <= C.PHASE_CAP
    assert good.mean() >= C.PHASE_SHARE, good.mean()
    e_ph = float(np.max(np.abs(res['phase_sum'] - ph)[good] / bound[good]))
    rest = res['phase_sum'][~good]
    assert np.all(np.isfinite(rest)) and np.all(np.abs(rest) <= ref.shape[0] + 1e-6)
    return e_ps, e_ph


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', C.DTYPES)
@pytest.mark.parametrize('n', C.SIZES)
def test_epoch_sums_at_every_support_edge(n, dtype, kind):
    worst = {'power_sum': (0.0, None), 'phase_sum': (0.0, None)}
    differ = []                                   # (out, K, max difference) of max_batch 2 against S
    for k in C.supports(n):
        res = {}
        for mb in (S, 2):
            p = make_plan(n, dtype, kind, k, mb)
            try:
                x, ref = case_reference(p, n, dtype, kind, k)
                for out in ('power_sum', 'phase_sum'):
                    got = np.array(p.execute(x, out_kind=out))
                    st = p.stats()
                    path = L.NW_REDUCE_PARTIALS if n in C.PARTIALS[dtype, out] else L.NW_REDUCE_ROWS
                    assert st['engine'] == 'fused' and st['reduce_path'] == path, (k, out, mb, st)
                    if out in res and not np.array_equal(got, res[out]):
                        differ.append((out, k, float(np.max(np.abs(got - res[out])))))
                    res[out] = got
            finally:
                p.close()
        assert res['power_sum'].dtype == np.float64 and res['phase_sum'].dtype == np.complex128
        for out, e in zip(('power_sum', 'phase_sum'), epoch_excess(res, ref, dtype)):
            if e > worst[out][0]:
                worst[out] = (e, k)
    for out, (e, k) in worst.items():
        print(f'B {kind} n={n} {dtype} {out}: worst err / bound {e:.3f} at K = {k}')
    assert not differ, f'max_batch = 2 and max_batch = {S} differ at {len(differ)} (out, K): {differ[:4]}'
    assert all(e <= 1.0 for e, _ in worst.values()), worst


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [n for n in C.SIZES if C.pair_kernel(n, 'float32')])
def test_pair_sums_around_the_kept_rows(n, kind):
    """cross_sum and plv_sum of the pairs (x0, x1), (x2, x3) as block partials of the pair kernel.
    With A_e, B_e the two channels' row maxima: |dS_ab| <= 2 TOL sum_e A_e B_e (each factor is
    off by TOL of its maximum), |dP_aa| <= 2 TOL sum_e A_e^2, and a product of two phasors by the
    sum of phase_sum's two bounds, where that is under the cap."""
    dtype, tol = 'float32', C.TOL['float32']
    worst = {'S_ab': 0.0, 'P_aa': 0.0, 'P_bb': 0.0, 'plv': 0.0}
    for k in C.pair_supports(n):
        p = make_plan(n, dtype, kind, k, S)
        try:
            x, ref = case_reference(p, n, dtype, kind, k)
            xa, xb = x[0::2][:2], x[1::2][:2]
            cross = np.array(p.execute_pair(xa, xb, out_kind='cross_sum'))
            st = p.stats()
            assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_pair_kernel', st
            assert st['reduce_path'] == L.NW_REDUCE_PARTIALS, (k, st)
            phi = np.array(p.execute_pair(xa, xb, out_kind='plv_sum'))
            assert p.stats()['reduce_path'] == L.NW_REDUCE_PARTIALS, (k, p.stats())
        finally:
            p.close()
        ya, yb = ref[0::2][:2], ref[1::2][:2]
        want, want_phi = C.pair_sums(ya, yb)
        A, B = C.row_max(ya), C.row_max(yb)                         # (2, F)
        ds = np.abs((cross[..., 0] + 1j * cross[..., 1]) - (want[..., 0] + 1j * want[..., 1]))
        worst['S_ab'] = max(worst['S_ab'], float(np.max(ds / (2 * tol * np.sum(A * B, axis=0))[:, None])))
        for name, c, m in (('P_aa', 2, A), ('P_bb', 3, B)):
            d = np.abs(cross[..., c] - want[..., c]) / (2 * tol * np.sum(m * m, axis=0))[:, None]
            worst[name] = max(worst[name], float(np.max(d)))
        bound = 2 * tol * np.sum(A[:, :, None] / np.abs(ya) + B[:, :, None] / np.abs(yb), axis=0)
        good = bound <= C.PHASE_CAP
        assert good.mean() >= 0.8, good.mean()
        worst['plv'] = max(worst['plv'], float(np.max(np.abs(phi - want_phi)[good] / bound[good])))
        assert np.all(np.isfinite(phi[~good])) and np.all(np.abs(phi[~good]) <= 2 + 1e-6)
    print(f'B pairs {kind} n={n}: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------ C. blocks of 8 signals
BIG_S, BIG_F = 67, 256
STARTS = [0, 2, 4, 6, 8, 30, 62, 64, 66]
HOST_SIGNALS, HOST_ROWS = [3, 66], [0, 1, 3, 10, 40, 100, 255]


@pytest.mark.parametrize('n,dtype,out', [(8192, 'float32', 'cwt'), (8192, 'float32', 'power'), (8192, 'float64', 'cwt'),
                                         (4096, 'float64', 'cwt'), (16384, 'float32', 'abs'),
                                         (16384, 'float32', 'power')])
def test_blocks_of_eight_signals(n, dtype, out):
    import torch
    dev = torch.device('cuda', 0)
    freqs = np.arange(1., BIG_F + 1)
    base = C.group_base(n, dtype)
    assert C.group_filling(base, BIG_S, BIG_F) == 8 and C.group_filling(base, 2, BIG_F) == 2
    assert BIG_S % 8 == 3                                           # the last block is ragged
    x = C.signals(n, dtype, BIG_S, C.nyquist_lead(BIG_S))      # the Nyquist bin differs inside every block of 8
    odt = {('cwt', 'float32'): torch.complex64, ('cwt', 'float64'): torch.complex128}.get(
        (out, dtype), torch.float32 if dtype == 'float32' else torch.float64)
    p = nw.Plan(n, BIG_F, dtype, max_batch=BIG_S)
    try:
        p.set_wavelet('morse', [17.5, 3.], freqs, L.trans_grid(n / 1000., 1000., False))
        xd = torch.from_numpy(np.array(x)).to(dev)
        big = torch.empty((BIG_S, BIG_F, n), dtype=odt, device=dev)
        p.execute(xd, big, out_kind=out)
        torch.cuda.synchronize()
        st = p.stats()
        assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'nw_fused_kernel', st
        assert st['launches_fused'] == 1, st
        for s0 in STARTS:
            cnt = min(2, BIG_S - s0)
            small = torch.empty((cnt, BIG_F, n), dtype=odt, device=dev)
            p.execute(xd[s0:s0 + cnt], small, out_kind=out)
            torch.cuda.synchronize()
            assert torch.equal(small, big[s0:s0 + cnt]), f'signals {s0}..{s0 + cnt - 1} alone differ from the launch of {BIG_S}'
            del small
        got = big[HOST_SIGNALS][:, HOST_ROWS].cpu().numpy()
        del big, xd
    finally:
        p.close()
        torch.cuda.empty_cache()
    want = np.stack([O.cwt('morse', x[s].astype(np.float64), freqs[HOST_ROWS]) for s in HOST_SIGNALS])
    e = row_excess(got, C.as_kind(want, out), dtype, out)
    print(f'C n={n} {dtype} {out}: worst err / bound {e.max():.3f} (per row {np.array2string(e.max(axis=0), precision=3)})')
    assert np.all(e <= 1.0), e
