"""Phase-amplitude coupling on device tensors (the library given by NINWAVE_LIB), NW_TIMING plans, warm-up,
the arms interleaved in one process, device time = the sum of the stage times of nw_plan_stats, wall time
around a synchronise.  No gate: what is measured is recorded (profiles/r16_pac_rate.txt).

C = 8 channels, every channel with itself (P = 8), E = 64 epochs x n = 4096, F = 64 Morse scales of which the
first 16 are the phase scales and the other 48 the amplitude scales, 128 signals per chunk, fp32 and fp64:
  (a) one Plan.execute_pac call (M, amp and phase) against one Plan.execute_conn_time(cross_sum) call over
      all 28 pairs on the same plan: the same rows from the same transform stage -- device, epilogue stage
      (the reduction kernels alone) and wall ms;
  (b) against the host route the call replaces: execute(..., 'cwt') to host memory plus the numpy formula
      (wall, one run);
  (c) the reduction stage against its algorithmic bytes -- the chunk's rows read once, C ec F n 2 esz; the
      sums written are 5 orders smaller -- as a fraction of 8 TB/s: nw_pac_kernel alone (no amp / phase
      outputs) and with nw_pac_rows_kernel (which reads the rows a second time).
    python tools/pac_rate.py [output file, default profiles/r16_pac_rate.txt]"""
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
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r16_pac_rate.txt')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run(dt):
    n, E, C, F, batch = 4096, 64, 8, 64, 128
    nph, nam = 16, 48
    fph, fam = np.arange(nph), np.arange(nph, nph + nam)
    esz = 4 if dt == 'float32' else 8
    tdt = torch.float32 if dt == 'float32' else torch.float64
    ia, ib = all_pairs(C)
    P = len(ia)
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    tm = torch.empty((E, C, nph, nam), device='cuda', dtype=torch.complex128)
    ta = torch.empty((E, C, nam, 2), device='cuda', dtype=torch.float64)
    tu = torch.empty((E, C, nph), device='cuda', dtype=torch.complex128)
    ts = torch.empty((E, P, F), device='cuda', dtype=torch.complex128)
    tp = torch.empty((E, C, F), device='cuda', dtype=torch.float64)

    def once(arm):
        if arm == 'pac':
            plan.execute_pac(x, None, fph, fam, out=(tm, ta, tu))
        elif arm == 'pac/m':
            plan.execute_pac(x, None, fph, fam, out=(tm, None, None))
        else:
            plan.execute_conn_time(x, (ia, ib), out=(ts, tp), out_kind='cross_sum')

    arms = ('pac', 'pac/m', 'conn_time')
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
    a, c = 'pac', 'conn_time'
    say('(a) %s n=%d C=%d E=%d F=%d, %d phase x %d amplitude scales, P=%d own-channel pairs: one execute_pac: device %.3f ms '
        '(median %.3f), of it the reduction (epilogue stage, %d chunks) %.3f ms (median %.3f), wall %.3f ms (median %.3f) | one '
        'execute_conn_time(cross_sum), %d pairs: device %.3f ms (median %.3f), reduction %.3f ms (median %.3f), wall %.3f ms '
        '(median %.3f) | pac / conn_time: device %.3fx reduction %.3fx wall %.3fx' % (
            dt, n, C, E, F, nph, nam, C, min(dev[a]), np.median(dev[a]), chunks, min(epi[a]), np.median(epi[a]), min(wall[a]),
            np.median(wall[a]), P, min(dev[c]), np.median(dev[c]), min(epi[c]), np.median(epi[c]), min(wall[c]),
            np.median(wall[c]), min(dev[a]) / min(dev[c]), min(epi[a]) / min(epi[c]), min(wall[a]) / min(wall[c])))
    # (b) the host route: every row over PCIe, then the numpy formula (one warm transform, one timed run)
    xh = x.cpu().numpy()
    plan.execute(xh.reshape(E * C, n), out_kind='cwt')
    t0 = time.perf_counter()
    y = plan.execute(xh.reshape(E * C, n), out_kind='cwt').reshape(E, C, F, n)
    t1 = time.perf_counter()
    A = np.abs(y[:, :, fam])
    u = y[:, :, fph] / np.abs(y[:, :, fph])
    res = [np.matmul(u, np.swapaxes(A, -1, -2).astype(u.dtype)), A.sum(-1), (A * A).sum(-1), u.sum(-1)]
    t2 = time.perf_counter()
    del y, A, u, res
    say('(b) %s the host route: execute(cwt) to host %.1f ms + numpy formula %.1f ms = wall %.1f ms | host route / '
        'execute_pac: wall %.0fx' % (dt, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3,
                                     (t2 - t0) * 1e3 / min(wall[a])))
    plan.close()
    # (c) the reduction stage against the rows read once
    rows = E * C * F * n * 2 * esz
    for k, what in (('pac/m', 'nw_pac_kernel alone'), ('pac', 'nw_pac_kernel + nw_pac_rows_kernel')):
        ms = min(epi[k])
        say('(c) %s %s: %.3f ms over %d launches (%.4f ms per epoch); the rows read once %.3f GB -> %.2f TB/s = %.1f %% of '
            '8 TB/s' % (dt, what, ms, chunks, ms / E, rows / 1e9, rows / ms / 1e9, 100 * rows / (ms * 1e-3) / HBM))


say('# tools/pac_rate.py on %s, %s' % (torch.cuda.get_device_name(0), os.environ.get('NINWAVE_LIB', 'libninwave.so')))
run('float32')
run('float64')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
