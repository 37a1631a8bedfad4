"""The timed launch paths give the untimed bits.

NW_TIMING launches the kernels of a stage through hipExtLaunchKernelGGL with the stage's
events (and NW_TIMING_CHAIN, the benchmark's mode, chains every stage onto the previous
one); without it they go through the plain launch.  Timing must not change what is computed:
for every engine form, three plans (untimed, timed, timed + chained) on the same seeded input
give byte-identical outputs (compared as raw bytes, so NaNs count), the same launch counters,
and stage times that are finite, non-negative and not all zero on the timed plans, all zero on
the untimed one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import REDUCTIONS, out_dtype  # noqa: E402

MORSE = ('morse', [17.5, 3.])
# id: (n, dtype, freqs, S, max_batch, out kinds, engine, wavelet)
CASES = {
    # the pair kernel and its partial-sum path; 5 signals in batches of 4: a full and a partial chunk
    'one_pass_f32': (1024, 'float32', np.linspace(2., 100., 8), 5, 4, ('cwt', 'power', 'power_mean', 'itc'), None, MORSE),
    'one_pass_f64': (1024, 'float64', np.linspace(2., 100., 8), 5, 4, ('cwt',), None, MORSE),   # single-signal kernel
    'chirp': (300, 'float32', np.linspace(2., 100., 6), 5, 4, ('power', 'power_sum'), None, MORSE),
    # on-chip rows, rocFFT overflow rows and expand (test_gpu_chirp.py::test_chirp_tentative_lengths)
    'hybrid_chirp': (10001, 'float32', np.array([2., 5., 400.]), 2, 2, ('cwt',), None, MORSE),
    'two_pass': (32768, 'float32', np.linspace(2., 100., 4), 2, 1, ('power',), None, MORSE),
    'rocfft': (1024, 'float32', np.linspace(2., 100., 8), 5, 4, ('cwt', 'abs', 'power_mean'), 'rocfft', MORSE),
    'repeated_rows': (1024, 'float32', np.linspace(2., 100., 4), 5, 4, ('cwt',), None, ('shannon', [])),   # U = 1: expand
}
MODES = ((False, False), (True, False), (True, True))   # (timing, timing_chain)


def signals(S, n, dtype):
    return np.random.default_rng(20).standard_normal((S, n)).astype(dtype)


def three_plans(case):
    n, dtype, freqs, _, max_batch, _, engine, (kind, params) = CASES[case]
    g = L.trans_grid(n / 1000., 1000., False)
    plans = []
    for timing, chain in MODES:
        p = nw.Plan(n, len(freqs), dtype, max_batch=max_batch, engine=engine, timing=timing, timing_chain=chain)
        p.set_wavelet(kind, params, freqs, g)
        plans.append(p)
    return plans


def check_stats(plans):
    stats = [p.stats() for p in plans]
    ms = [[v for k, v in st.items() if k.startswith('ms_')] for st in stats]
    print('ms sums (untimed, timed, chained):', [sum(m) for m in ms])
    assert all(v == 0 for v in ms[0])
    for m in ms[1:]:
        assert all(np.isfinite(v) and v >= 0 for v in m)
        assert sum(m) > 0
    same = [k for k in stats[0] if k.startswith('launches_')] + ['chunks', 'kernel', 'unique_rows']
    for st in stats[1:]:
        assert {k: st[k] for k in same} == {k: stats[0][k] for k in same}


@pytest.mark.parametrize('case', list(CASES))
def test_timed_outputs_equal_untimed_from_host_arrays(case):
    n, dtype, _, S, _, outs, _, _ = CASES[case]
    x = signals(S, n, dtype)
    plans = three_plans(case)
    for out in outs:
        got = [p.execute(x, out_kind=out).tobytes() for p in plans]
        assert got[1] == got[0], (out, 'timed')
        assert got[2] == got[0], (out, 'timed + chained')
    check_stats(plans)


def device_execute(torch, p, xt, out):
    n, F = p.n, p.nfreq
    shape = (F, n) if out in REDUCTIONS else (xt.shape[0], F, n)
    ot = torch.empty(shape, dtype=getattr(torch, np.dtype(out_dtype(p.dtype, out)).name), device='cuda')
    p.execute(xt, ot, out_kind=out)
    return ot


@pytest.mark.parametrize('case', ['one_pass_f32', 'two_pass', 'rocfft'])
def test_timed_outputs_equal_untimed_from_device_tensors(case):
    torch = pytest.importorskip('torch')
    n, dtype, _, S, _, outs, _, _ = CASES[case]
    xt = torch.from_numpy(signals(S, n, dtype)).cuda()
    plans = three_plans(case)
    for out in outs:
        ots = [device_execute(torch, p, xt, out) for p in plans]
        for p in plans:
            p.sync()
        got = [o.cpu().numpy().tobytes() for o in ots]
        assert got[1] == got[0], (out, 'timed')
        assert got[2] == got[0], (out, 'timed + chained')
    check_stats(plans)


def test_chained_plan_closed_with_stages_pending():
    """Device-memory executes leave their stage events pending until sync() or stats(); a
    chained stage's start event is the previous stage's stop event, and closing the plan
    releases each event once.  A fresh plan then computes the same bits."""
    torch = pytest.importorskip('torch')
    case = 'one_pass_f32'
    n, dtype, freqs, S, max_batch, _, _, (kind, params) = CASES[case]
    g = L.trans_grid(n / 1000., 1000., False)
    xt = torch.from_numpy(signals(S, n, dtype)).cuda()
    p = nw.Plan(n, len(freqs), dtype, max_batch=max_batch, timing=True, timing_chain=True)
    p.set_wavelet(kind, params, freqs, g)
    first = device_execute(torch, p, xt, 'cwt')
    second = device_execute(torch, p, xt, 'cwt')
    p.close()                                     # waits for the stream, no sync() / stats() before
    q = nw.Plan(n, len(freqs), dtype, max_batch=max_batch)
    q.set_wavelet(kind, params, freqs, g)
    ref = device_execute(torch, q, xt, 'cwt')
    q.sync()
    want = ref.cpu().numpy().tobytes()
    assert first.cpu().numpy().tobytes() == want and second.cpu().numpy().tobytes() == want
