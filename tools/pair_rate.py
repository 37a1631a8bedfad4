"""Cross-channel pair reductions on device tensors (the library given by NINWAVE_LIB): cross_sum
and plv_sum of 512 epochs x 256 Morse scales against the complex CWT of the same 1024 interleaved
signals (what a caller without the reductions has to produce before numpy), per n and dtype, the
arms interleaved in one process, NW_TIMING stage sums and wall times.  Each reduction runs twice:
as the plan chooses (nw_stats.reduce_path 2 where nw_pair_partials_supported: block partials in
the kernel) and with NW_NO_PAIR_PARTIALS set (path 1: the chunk's rows through k_accumulate_pair).
    DTYPES="float32 float64" NS="1024 2048 4096" python tools/pair_rate.py [tag]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L

STAGES = ('ms_forward', 'ms_multiply', 'ms_inverse', 'ms_epilogue', 'ms_fused', 'ms_copy', 'ms_rows', 'ms_expand')
tag = sys.argv[1] if len(sys.argv) > 1 else ''
for dt in os.environ.get('DTYPES', 'float32 float64').split():
    tdt = torch.float32 if dt == 'float32' else torch.float64
    cdt = torch.complex64 if dt == 'float32' else torch.complex128
    for n in [int(v) for v in os.environ.get('NS', '1024 2048 4096').split()]:
        E, F, C = 512, 256, 128          # pairs, scales, signals per chunk (64 pairs)
        plan = nw.Plan(n, F, dt, max_batch=C, timing=True)
        plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
        a = torch.randn((E, n), device='cuda', dtype=tdt)
        b = 0.6 * a + 0.8 * torch.randn((E, n), device='cuda', dtype=tdt)
        inter = torch.stack([a, b], dim=1).reshape(2 * E, n).contiguous()
        oc = torch.empty((F, n, 4), device='cuda', dtype=torch.float64)
        op = torch.empty((F, n), device='cuda', dtype=torch.complex128)
        oy = torch.empty((C, F, n), device='cuda', dtype=cdt)

        def once(kind):
            os.environ.pop('NW_NO_PAIR_PARTIALS', None)
            if kind.endswith('/rows'):
                os.environ['NW_NO_PAIR_PARTIALS'] = '1'
                kind = kind[:-5]
            if kind == 'cwt':
                for s0 in range(0, 2 * E, C):
                    plan.execute(inter[s0:s0 + C], oy, out_kind='cwt')
            else:
                plan.execute_pair(a, b, out=oc if kind == 'cross_sum' else op, out_kind=kind)

        kinds = ('cross_sum', 'cross_sum/rows', 'plv_sum', 'plv_sum/rows', 'cwt')
        wall = {k: [] for k in kinds}
        dev = {k: [] for k in kinds}
        path = {}
        for k in kinds:
            once(k); plan.sync(); torch.cuda.synchronize()
        for _ in range(5):               # interleaved: every arm sees the same clocks
            for k in kinds:
                plan.reset_stats()
                t0 = time.perf_counter(); once(k); plan.sync(); torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                st = plan.stats()
                dev[k].append(sum(st[s] for s in STAGES))
                path[k] = st['reduce_path'] if k != 'cwt' else 0
        pts = 2 * E * F * n
        w = {k: min(v) for k, v in wall.items()}
        d = {k: min(v) for k, v in dev.items()}
        for k in ('cross_sum', 'plv_sum'):
            print('%s %s n=%5d %-9s path %d: stages %.3f ms wall %.3f ms (%.3e pts/s, %.2fx cwt) | path %d: stages %.3f ms '
                  'wall %.3f ms (%.2fx cwt) | partials/rows %.3f | cwt stages %.3f ms' % (
                      tag, dt, n, k, path[k], d[k], w[k], pts / w[k] * 1e3, d[k] / d['cwt'], path[k + '/rows'],
                      d[k + '/rows'], w[k + '/rows'], d[k + '/rows'] / d['cwt'], d[k] / d[k + '/rows'], d['cwt']), flush=True)
        plan.close()
