"""Multi-channel connectivity on device tensors (the library given by NINWAVE_LIB), NW_TIMING plans,
warm-up, the arms interleaved in one process, device time = the sum of the stage times of
nw_plan_stats, wall time around a synchronise.

A  one Plan.execute_conn call over all pairs of C = 8 channels (E = 64 epochs, F = 64 Morse scales)
   against the 28 Plan.execute_pair calls that give the same sums, the same plan and so the same
   signals per chunk (128) in both: fp32 n = 4096 (the gate: the single call is faster on both
   clocks, cross_sum and plv_sum), then fp64 n = 4096 and fp32 n = 1201 for the record.
B  nw_conn_accumulate_kernel alone (cross_sum without power sums: the epilogue stage is that one
   kernel) per launch at C = 32, all 496 pairs, fp32, n = 4096, F = 64, ec epochs per chunk, against
   its algorithmic bytes -- the chunk's rows read once, C ec F n 8 B, plus the accumulators read and
   written, 2 P F n 16 B -- as a fraction of 8 TB/s, in both block orders (XCD-aware, conn_slot;
   NW_CONN_PLAIN_ORDER: plain).
C  the phase-lag sums (out_kind lag_sum), no gate: at A's fp32 n = 4096 shapes one
   execute_conn(lag_sum) against execute_conn(cross_sum) of the same plan and against the 28
   execute_pair(lag_sum) calls; at B's shapes the kernel's lag mode per launch against its algorithmic
   bytes, the chunk's rows read once plus 2 P F n 32 B of accumulators (recorded in
   profiles/r14_lag_rate.txt).
D  over-time connectivity (Plan.execute_conn_time, recorded in profiles/r15_conn_time_rate.txt), no gate:
   at A's shapes, fp32 and fp64 n = 4096, one execute_conn_time(cross_sum) and one execute_conn_time(lag_sum)
   against (a) execute_conn of the same kind on the same plan, which reads the same rows -- device, epilogue
   stage (the reduction kernels alone) and wall ms -- and (b) the host route the call replaces: execute(...,
   'cwt') to host memory plus the numpy reduction over the samples (wall, one run).  Then the reduction
   kernels alone at 2 epochs per chunk (a grid of only ec F ntiles blocks) against A's 16.
    [EC="2 8 32"] python tools/conn_rate.py [output file, default profiles/r12_conn_rate.txt] [A|B|AB|C|D]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import all_pairs

STAGES = ('ms_forward', 'ms_multiply', 'ms_inverse', 'ms_epilogue', 'ms_fused', 'ms_copy', 'ms_rows', 'ms_expand')
HBM = 8e12
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r12_conn_rate.txt')
parts = sys.argv[2] if len(sys.argv) > 2 else 'AB'
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def algorithmic_bytes(C, P, F, n, ec, esz):
    """rows of the chunk read once + the cross accumulators read and written"""
    return C * ec * F * n * 2 * esz + 2 * P * F * n * 16


def timed(plan, fn, reps, arms):
    """min and median over reps of (device ms, wall ms) per arm, the arms interleaved"""
    dev = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    for k in arms:
        fn(k); plan.sync(); torch.cuda.synchronize()
    for _ in range(reps):
        for k in arms:
            plan.reset_stats()
            t0 = time.perf_counter(); fn(k); plan.sync(); torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            st = plan.stats()
            dev[k].append(sum(st[s] for s in STAGES))
    return {k: (min(dev[k]), float(np.median(dev[k])), min(wall[k]), float(np.median(wall[k]))) for k in arms}


def part_a(dt, n, gate):
    E, C, F, batch = 64, 8, 64, 128
    tdt = torch.float32 if dt == 'float32' else torch.float64
    ia, ib = all_pairs(C)
    P = len(ia)
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    chans = [x[:, c].contiguous() for c in range(C)]            # the pair calls' inputs, made outside the clock
    oc = torch.empty((P, F, n), device='cuda', dtype=torch.complex128)
    opw = torch.empty((C, F, n), device='cuda', dtype=torch.float64)
    pc = torch.empty((F, n, 4), device='cuda', dtype=torch.float64)
    pp = torch.empty((F, n), device='cuda', dtype=torch.complex128)

    def once(arm):
        kind, how = arm.split('/')
        if how == 'conn':
            plan.execute_conn(x, (ia, ib), out=(oc, opw) if kind == 'cross_sum' else oc, out_kind=kind)
        else:
            for a, b in zip(ia, ib):
                plan.execute_pair(chans[a], chans[b], out=pc if kind == 'cross_sum' else pp, out_kind=kind)

    arms = ('cross_sum/conn', 'cross_sum/pairs', 'plv_sum/conn', 'plv_sum/pairs')
    r = timed(plan, once, 5, arms)
    once('cross_sum/pairs')
    path = plan.stats()['reduce_path']
    plan.close()
    ok = True
    for kind in ('cross_sum', 'plv_sum'):
        c, p = r[kind + '/conn'], r[kind + '/pairs']
        say('A %s n=%d C=%d E=%d F=%d %-9s one execute_conn: device %.3f ms (median %.3f) wall %.3f ms (median %.3f) | '
            '%d execute_pair (reduce_path %d): device %.3f ms (median %.3f) wall %.3f ms (median %.3f) | '
            'pairs / conn: device %.2fx wall %.2fx' % (dt, n, C, E, F, kind, c[0], c[1], c[2], c[3], P, path, p[0], p[1],
                                                        p[2], p[3], p[0] / c[0], p[2] / c[2]))
        ok = ok and c[0] < p[0] and c[2] < p[2]
    if gate:
        say('A gate (%s n=%d: the single call faster on both clocks, both kinds): %s' % (dt, n, 'PASS' if ok else 'FAIL'))
    return ok


def part_b(ec):
    dt, n, F, C = 'float32', 4096, 64, 32
    ia, ib = all_pairs(C)
    P = len(ia)
    E = 2 * ec                                                      # two launches per call
    plan = nw.Plan(n, F, dt, max_batch=ec * C, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    x = torch.randn((E, C, n), device='cuda', dtype=torch.float32)
    oc = torch.empty((P, F, n), device='cuda', dtype=torch.complex128)
    ms = {}
    for order in ('xcd', 'plain'):
        os.environ.pop('NW_CONN_PLAIN_ORDER', None)
        if order == 'plain':
            os.environ['NW_CONN_PLAIN_ORDER'] = '1'
        best = []
        for rep in range(4):
            plan.reset_stats()
            plan.execute_conn(x, (ia, ib), out=(oc, None), out_kind='cross_sum'); plan.sync()
            st = plan.stats()
            if rep:
                best.append(st['ms_epilogue'] / st['chunks'])
        ms[order] = min(best)
    os.environ.pop('NW_CONN_PLAIN_ORDER', None)
    plan.close()
    nbytes = algorithmic_bytes(C, P, F, n, ec, 4)
    ntiles = L.conn_tiles(C, ia, ib)[1]
    for order in ('xcd', 'plain'):
        say('B fp32 n=%d F=%d C=%d P=%d (%d tiles) ec=%d %-5s order: nw_conn_accumulate_kernel %.3f ms per launch, '
            '%.3f ms per epoch; algorithmic %.3f GB (rows %.3f + accumulators %.3f) -> %.2f TB/s = %.1f %% of 8 TB/s' % (
                n, F, C, P, ntiles, ec, order, ms[order], ms[order] / ec, nbytes / 1e9, C * ec * F * n * 8 / 1e9,
                2 * P * F * n * 16 / 1e9, nbytes / ms[order] / 1e9, 100 * nbytes / (ms[order] * 1e-3) / HBM))


def part_c_calls():
    dt, n, E, C, F, batch = 'float32', 4096, 64, 8, 64, 128
    ia, ib = all_pairs(C)
    P = len(ia)
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=torch.float32)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=torch.float32)).contiguous()
    chans = [x[:, c].contiguous() for c in range(C)]
    oc = torch.empty((P, F, n), device='cuda', dtype=torch.complex128)
    opw = torch.empty((C, F, n), device='cuda', dtype=torch.float64)
    ol = torch.empty((P, F, n, 4), device='cuda', dtype=torch.float64)
    pl = torch.empty((F, n, 4), device='cuda', dtype=torch.float64)

    def once(arm):
        if arm == 'lag_sum/conn':
            plan.execute_conn(x, (ia, ib), out=ol, out_kind='lag_sum')
        elif arm == 'cross_sum/conn':
            plan.execute_conn(x, (ia, ib), out=(oc, opw), out_kind='cross_sum')
        else:
            for a, b in zip(ia, ib):
                plan.execute_pair(chans[a], chans[b], out=pl, out_kind='lag_sum')

    r = timed(plan, once, 5, ('lag_sum/conn', 'cross_sum/conn', 'lag_sum/pairs'))
    once('lag_sum/pairs')
    path = plan.stats()['reduce_path']
    plan.close()
    lag, cross, pairs = r['lag_sum/conn'], r['cross_sum/conn'], r['lag_sum/pairs']
    say('C %s n=%d C=%d E=%d F=%d one execute_conn lag_sum: device %.3f ms (median %.3f) wall %.3f ms (median %.3f) | '
        'cross_sum: device %.3f ms (median %.3f) wall %.3f ms (median %.3f) | lag / cross: device %.2fx wall %.2fx' % (
            dt, n, C, E, F, lag[0], lag[1], lag[2], lag[3], cross[0], cross[1], cross[2], cross[3], lag[0] / cross[0],
            lag[2] / cross[2]))
    say('C %s n=%d C=%d E=%d F=%d one execute_conn lag_sum | %d execute_pair lag_sum (reduce_path %d): device %.3f ms '
        '(median %.3f) wall %.3f ms (median %.3f) | pairs / conn: device %.2fx wall %.2fx' % (
            dt, n, C, E, F, P, path, pairs[0], pairs[1], pairs[2], pairs[3], pairs[0] / lag[0], pairs[2] / lag[2]))


def part_c_kernel(ec):
    dt, n, F, C = 'float32', 4096, 64, 32
    ia, ib = all_pairs(C)
    P = len(ia)
    E = 2 * ec                                                      # two launches per call
    plan = nw.Plan(n, F, dt, max_batch=ec * C, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    x = torch.randn((E, C, n), device='cuda', dtype=torch.float32)
    ol = torch.empty((P, F, n, 4), device='cuda', dtype=torch.float64)
    best = []
    for rep in range(4):
        plan.reset_stats()
        plan.execute_conn(x, (ia, ib), out=ol, out_kind='lag_sum'); plan.sync()
        st = plan.stats()
        if rep:
            best.append(st['ms_epilogue'] / st['chunks'])
    plan.close()
    ms = min(best)
    rows, accs = C * ec * F * n * 8, 2 * P * F * n * 32
    say('C fp32 n=%d F=%d C=%d P=%d (%d tiles) ec=%d: nw_conn_accumulate_kernel (lag) %.3f ms per launch, %.3f ms per '
        'epoch; algorithmic %.3f GB (rows %.3f + accumulators %.3f) -> %.2f TB/s = %.1f %% of 8 TB/s' % (
            n, F, C, P, L.conn_tiles(C, ia, ib)[1], ec, ms, ms / ec, (rows + accs) / 1e9, rows / 1e9, accs / 1e9,
            (rows + accs) / ms / 1e9, 100 * (rows + accs) / (ms * 1e-3) / HBM))


def part_d(dt):
    n, E, C, F, batch = 4096, 64, 8, 64, 128
    tdt = torch.float32 if dt == 'float32' else torch.float64
    ia, ib = all_pairs(C)
    P = len(ia)
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    oc = torch.empty((P, F, n), device='cuda', dtype=torch.complex128)
    opw = torch.empty((C, F, n), device='cuda', dtype=torch.float64)
    ol = torch.empty((P, F, n, 4), device='cuda', dtype=torch.float64)
    ts = torch.empty((E, P, F), device='cuda', dtype=torch.complex128)
    tp = torch.empty((E, C, F), device='cuda', dtype=torch.float64)
    tl = torch.empty((E, P, F, 4), device='cuda', dtype=torch.float64)

    def once(arm):
        kind, how = arm.split('/')
        if how == 'time':
            plan.execute_conn_time(x, (ia, ib), out=(ts, tp) if kind == 'cross_sum' else tl, out_kind=kind)
        else:
            plan.execute_conn(x, (ia, ib), out=(oc, opw) if kind == 'cross_sum' else ol, out_kind=kind)

    arms = ('cross_sum/time', 'cross_sum/conn', 'lag_sum/time', 'lag_sum/conn')
    dev, epi, wall = ({k: [] for k in arms} for _ in range(3))
    for k in arms:
        once(k); plan.sync(); torch.cuda.synchronize()
    for _ in range(7):
        for k in arms:
            plan.reset_stats()
            t0 = time.perf_counter(); once(k); plan.sync(); torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            st = plan.stats()
            dev[k].append(sum(st[s] for s in STAGES))
            epi[k].append(st['ms_epilogue'])
    chunks = st['chunks']
    for kind in ('cross_sum', 'lag_sum'):
        t, c = kind + '/time', kind + '/conn'
        say('D %s n=%d C=%d P=%d E=%d F=%d %-9s one execute_conn_time: device %.3f ms (median %.3f), of it the reduction '
            '(epilogue stage, %d launches) %.3f ms (median %.3f), wall %.3f ms (median %.3f) | (a) one execute_conn: device '
            '%.3f ms (median %.3f), reduction %.3f ms (median %.3f), wall %.3f ms (median %.3f) | time / conn: device '
            '%.3fx reduction %.3fx wall %.3fx' % (
                dt, n, C, P, E, F, kind, min(dev[t]), np.median(dev[t]), chunks, min(epi[t]), np.median(epi[t]),
                min(wall[t]), np.median(wall[t]), min(dev[c]), np.median(dev[c]), min(epi[c]), np.median(epi[c]),
                min(wall[c]), np.median(wall[c]), min(dev[t]) / min(dev[c]), min(epi[t]) / min(epi[c]),
                min(wall[t]) / min(wall[c])))
    # (b) the host route: every row over PCIe, then numpy sums over the samples (one warm transform, one timed run)
    xh = x.cpu().numpy()
    plan.execute(xh.reshape(E * C, n), out_kind='cwt')
    for kind in ('cross_sum', 'lag_sum'):
        t0 = time.perf_counter()
        y = plan.execute(xh.reshape(E * C, n), out_kind='cwt').reshape(E, C, F, n)
        t1 = time.perf_counter()
        if kind == 'cross_sum':
            res = [np.stack([np.einsum('eft,eft->ef', y[:, a], np.conj(y[:, b])) for a, b in zip(ia, ib)], axis=1),
                   np.einsum('ecft,ecft->ecf', y.real, y.real) + np.einsum('ecft,ecft->ecf', y.imag, y.imag)]
        else:
            res = []
            for a, b in zip(ia, ib):
                m = y[:, a].imag * y[:, b].real - y[:, a].real * y[:, b].imag
                res.append(np.stack([m.sum(-1), np.abs(m).sum(-1), (m * m).sum(-1), np.sign(m).sum(-1)], axis=-1))
        t2 = time.perf_counter()
        del y, res
        say('D %s n=%d C=%d P=%d E=%d F=%d %-9s (b) the host route: execute(cwt) to host %.1f ms + numpy reduction %.1f ms = '
            'wall %.1f ms | host route / execute_conn_time: wall %.0fx' % (
                dt, n, C, P, E, F, kind, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3,
                (t2 - t0) * 1e3 / min(wall[kind + '/time'])))
    plan.close()
    # the reduction kernels alone per launch: 16 epochs per chunk (above) and 2
    per16 = {k: min(epi[k + '/time']) / chunks for k in ('cross_sum', 'lag_sum')}
    small = nw.Plan(n, F, dt, max_batch=2 * C, timing=True)
    small.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    x4 = x[:4].contiguous()
    for kind in ('cross_sum', 'lag_sum'):
        best = []
        for rep in range(6):
            small.reset_stats()
            small.execute_conn_time(x4, (ia, ib), out=(ts[:4], None) if kind == 'cross_sum' else tl[:4], out_kind=kind)
            small.sync()
            st = small.stats()
            if rep:
                best.append(st['ms_epilogue'] / st['chunks'])
        rows = 2 * C * F * n * 2 * (4 if dt == 'float32' else 8)
        say('D %s n=%d C=%d P=%d F=%d %-9s nw_conn_time_kernel alone, ec=2 (%d blocks): %.4f ms per launch, %.4f ms per '
            'epoch, rows %.4f GB -> %.2f TB/s | ec=16 (%d blocks, with the power kernel for cross_sum): %.4f ms per launch, '
            '%.4f ms per epoch' % (dt, n, C, P, F, kind, 2 * F * L.conn_tiles(C, ia, ib)[1], min(best), min(best) / 2,
                                   rows / 1e9, rows / min(best) / 1e9, 16 * F * L.conn_tiles(C, ia, ib)[1], per16[kind],
                                   per16[kind] / 16))
    small.close()


say('# tools/conn_rate.py on %s, %s' % (torch.cuda.get_device_name(0), os.environ.get('NINWAVE_LIB', 'libninwave.so')))
gate = True
if 'A' in parts:
    gate = part_a('float32', 4096, True)
    part_a('float64', 4096, False)
    part_a('float32', 1201, False)
if 'B' in parts:
    for ec in [int(v) for v in os.environ.get('EC', '2 8 32').split()]:
        part_b(ec)
if 'C' in parts:
    part_c_calls()
    for ec in [int(v) for v in os.environ.get('EC', '2 8 32').split()]:
        part_c_kernel(ec)
if 'D' in parts:
    part_d('float32')
    part_d('float64')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
sys.exit(0 if gate else 1)
