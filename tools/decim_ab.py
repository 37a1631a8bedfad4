"""Interleaved same-process A/B of the decimated kernel against the full one (diagnostic):
per shape, one plan without decim (nw_fused_kernel / nw_fused_pair_kernel) and one per decim
(nw_fused_decim_kernel) on the same device-resident signals, executed in turn; the per-launch
time is NW_TIMING's ms_fused / launches_fused.  Prints one line per (shape, decim) and the
condition of DESIGN.md §4 Round 8: a decimated launch no slower than the full launch.
    python tools/decim_ab.py [--reps 5] [--shapes c4f32,c4f64,c3,all] > profiles/r08_decim_ab.txt
    python tools/decim_ab.py --host        (host numpy cwt_batch with decim=4 against full + slice)"""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

FREQS = np.arange(1, 257, dtype=np.float64)
SHAPES = {
    # name: (signals per launch, n, dtype, out kind, decims)
    'c4f32': (512, 16384, 'float32', 'cwt', (2, 4, 8, 16)),
    'c4f64': (512, 16384, 'float64', 'cwt', (2, 4, 8, 16)),
    'c3': (1024, 4096, 'float32', 'power', (2, 4)),
}
# every other supported (n, decim, dtype): 256 signals x 256 Morse scales, cwt
for _n in (2048, 4096, 8192):
    for _dt in ('float32', 'float64'):
        SHAPES[f'n{_n}{_dt[-2:]}'] = (256, _n, _dt, 'cwt', tuple(d for d in (2, 4, 8) if _n // d >= 1024))


def make_plan(S, n, dtype, decim):
    p = nw.Plan(n, len(FREQS), dtype, max_batch=S, timing=True, decim=decim)
    p.set_wavelet('morse', [17.5, 3.], FREQS, L.trans_grid(n / 1000., 1000., False))
    return p


def run(name, reps):
    S, n, dtype, out, decims = SHAPES[name]
    tdt = torch.float32 if dtype == 'float32' else torch.float64
    odt = tdt if out != 'cwt' else (torch.complex64 if dtype == 'float32' else torch.complex128)
    x = torch.randn((S, n), dtype=tdt, device='cuda')
    buf = torch.empty((S, len(FREQS), n), dtype=odt, device='cuda')
    plans = {d: make_plan(S, n, dtype, d) for d in (1,) + tuple(decims)}
    outs = {d: buf.view(-1)[:S * len(FREQS) * (n // d)].view(S, len(FREQS), n // d) for d in plans}
    for d, p in plans.items():                       # warm-up: W table, twiddles
        p.execute(x, outs[d], out_kind=out)
        p.sync()
        p.reset_stats()
    for _ in range(reps):
        for d, p in plans.items():
            p.execute(x, outs[d], out_kind=out)
            p.sync()
    ms = {}
    for d, p in plans.items():
        st = p.stats()
        ms[d] = st['ms_fused'] / st['launches_fused']
        kern = L.KERNEL_NAMES[st['kernel']]
        pts = S * len(FREQS) * (n // d) / (ms[d] * 1e-3)
        verdict = '' if d == 1 else ('  ok' if ms[d] <= ms[1] else '  SLOWER THAN FULL')
        print(f'{name:<8} {S} x {n} x {len(FREQS)} {dtype} {out:<5} decim {d:>2}: {ms[d]:8.4f} ms per launch '
              f'({st["launches_fused"]} launches), {pts:.3e} output points/s, x{ms[1] / ms[d]:.2f} vs full  {kern}{verdict}',
              flush=True)
        p.close()
    return all(ms[d] <= ms[1] for d in decims)


def host(reps, decim=4):
    """End to end through host arrays at the C2 shape (tools/host_rate.py's): cwt_batch(decim=4)
    against the full result sliced on the host."""
    import time
    S, n, F = 64, 16384, 128
    x = np.random.default_rng(0).standard_normal((S, n)).astype('float32')
    freqs = np.arange(1, F + 1, dtype=np.float64)
    w = nw.Morlet(1000, dtype='float32')
    arms = {'full + host slice': lambda: np.ascontiguousarray(w.cwt_batch(x, freqs)[..., ::decim]),
            f'decim={decim}': lambda: w.cwt_batch(x, freqs, decim=decim)}
    el = dict.fromkeys(arms, 0.0)
    for fn in arms.values():
        fn()                                       # warm-up: plans, W tables, pooled buffers
    for _ in range(reps):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            out = fn()
            el[k] += time.perf_counter() - t0
            del out
    for k in arms:
        print(f'host C2 64 x 16384 x 128 Morlet float32 cwt_batch, {k:<18}: {el[k] / reps * 1e3:8.2f} ms per call, '
              f'{S * F * (n // decim) / (el[k] / reps):.3e} kept points/s', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='c4f32,c4f64,c3')
    ap.add_argument('--host', action='store_true', help='only the end-to-end host cwt_batch comparison')
    a = ap.parse_args()
    if a.host:
        return host(a.reps)
    names = list(SHAPES) if a.shapes == 'all' else a.shapes.split(',')
    ok = [run(nm, a.reps) for nm in names]
    print('condition (every decimated launch no slower than the full launch):', 'holds' if all(ok) else 'FAILS')


if __name__ == '__main__':
    main()
