"""Event-related phase-amplitude coupling on device tensors (the library given by NINWAVE_LIB), NW_TIMING plans,
warm-up, the arms interleaved in one process, device time = the sum of the stage times of nw_plan_stats, wall time
around a synchronise.  No gate: what is measured is recorded (profiles/r20_erpac_rate.txt).

C = 8 channels, every channel with itself (P = 8), E = 64 epochs x n = 4096, F = 64 Morse scales of which the first
16 are the phase scales and the other 48 the amplitude scales, the window every 4th sample (T = 1024), at 2, 8 and 32
epochs per chunk (16, 64 and 256 signals), fp32 and fp64:
  (a) one Plan.execute_erpac call (M, amp and phase) against one Plan.execute_pac call over the same window on the
      same plan: the same rows from the same transform stage -- device, epilogue stage (the reduction kernels
      alone) and wall ms;
  (b) against the host route the call replaces: execute(..., 'cwt') to host memory plus the numpy formula (wall,
      one run);
  (c) the reduction stage against its algorithmic bytes -- the rows read once, C E F n 2 esz, plus the fp64
      accumulators (M, amp, phase) read and written once per chunk -- as a fraction of 8 TB/s: nw_erpac_kernel
      alone (no amp / phase outputs) and with nw_erpac_rows_kernel (which reads the rows a second time).
    python tools/erpac_rate.py [output file, default profiles/r20_erpac_rate.txt]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L

STAGES = ('ms_forward', 'ms_multiply', 'ms_inverse', 'ms_epilogue', 'ms_fused', 'ms_copy', 'ms_rows', 'ms_expand')
HBM = 8e12
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r20_erpac_rate.txt')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run(dt, per_chunk, host_route):
    n, E, C, F = 4096, 64, 8, 64
    nph, nam, step = 16, 48, 4
    T = n // step
    fph, fam = np.arange(nph), np.arange(nph, nph + nam)
    esz = 4 if dt == 'float32' else 8
    tdt = torch.float32 if dt == 'float32' else torch.float64
    plan = nw.Plan(n, F, dt, max_batch=per_chunk * C, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    torch.manual_seed(20)
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    em = torch.empty((C, nph, nam, T), device='cuda', dtype=torch.complex128)
    ea = torch.empty((C, nam, T, 2), device='cuda', dtype=torch.float64)
    eu = torch.empty((C, nph, 5, T), device='cuda', dtype=torch.float64)
    tm = torch.empty((E, C, nph, nam), device='cuda', dtype=torch.complex128)
    ta = torch.empty((E, C, nam, 2), device='cuda', dtype=torch.float64)
    tu = torch.empty((E, C, nph), device='cuda', dtype=torch.complex128)

    def once(arm):
        if arm == 'erpac':
            plan.execute_erpac(x, None, fph, fam, (0, n), step, out=(em, ea, eu))
        elif arm == 'erpac/m':
            plan.execute_erpac(x, None, fph, fam, (0, n), step, out=(em, None, None))
        else:
            plan.execute_pac(x, None, fph, fam, (0, n), step, out=(tm, ta, tu))

    arms = ('erpac', 'erpac/m', 'pac')
    dev, epi, wall = ({k: [] for k in arms} for _ in range(3))
    for k in arms:
        once(k); plan.sync(); torch.cuda.synchronize()
    for _ in range(5):
        for k in arms:
            plan.reset_stats()
            t0 = time.perf_counter(); once(k); plan.sync(); torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            st = plan.stats()
            dev[k].append(sum(st[s] for s in STAGES))
            epi[k].append(st['ms_epilogue'])
    chunks = st['chunks']
    a, c = 'erpac', 'pac'
    say('(a) %s n=%d C=%d E=%d F=%d, %d phase x %d amplitude scales, P=%d own-channel pairs, T=%d (every %dth sample), %d '
        'epochs per chunk: one execute_erpac: device %.3f ms (median %.3f), of it the reduction (epilogue stage, %d chunks) '
        '%.3f ms (median %.3f), wall %.3f ms (median %.3f) | one execute_pac: device %.3f ms (median %.3f), reduction %.3f '
        'ms (median %.3f), wall %.3f ms (median %.3f) | erpac / pac: device %.3fx reduction %.3fx wall %.3fx' % (
            dt, n, C, E, F, nph, nam, C, T, step, per_chunk, min(dev[a]), np.median(dev[a]), chunks, min(epi[a]),
            np.median(epi[a]), min(wall[a]), np.median(wall[a]), min(dev[c]), np.median(dev[c]), min(epi[c]),
            np.median(epi[c]), min(wall[c]), np.median(wall[c]), min(dev[a]) / min(dev[c]), min(epi[a]) / min(epi[c]),
            min(wall[a]) / min(wall[c])))
    # (c) the reduction stage against the rows read once and the accumulators moved twice per chunk
    rows = E * C * F * n * 2 * esz
    acc_m = C * nph * nam * T * 16
    acc_rows = C * nam * T * 16 + C * nph * 5 * T * 8
    for k, what, acc in (('erpac/m', 'nw_erpac_kernel alone', acc_m),
                         ('erpac', 'nw_erpac_kernel + nw_erpac_rows_kernel', acc_m + acc_rows)):
        ms = min(epi[k])
        total = rows + 2 * chunks * acc
        say('(c) %s %d epochs per chunk, %s: %.3f ms over %d chunks (%.4f ms per epoch); the rows read once %.3f GB + the '
            'accumulators twice per chunk %.3f GB -> %.2f TB/s = %.1f %% of 8 TB/s' % (
                dt, per_chunk, what, ms, chunks, ms / E, rows / 1e9, 2 * chunks * acc / 1e9, total / ms / 1e9,
                100 * total / (ms * 1e-3) / HBM))
    if host_route:
        # (b) the host route: every row over PCIe, then the numpy formula (one warm transform, one timed run)
        xh = x.cpu().numpy()
        plan.execute(xh.reshape(E * C, n), out_kind='cwt')
        t0 = time.perf_counter()
        y = plan.execute(xh.reshape(E * C, n), out_kind='cwt').reshape(E, C, F, n)[..., ::step]
        t1 = time.perf_counter()
        A = np.abs(y[:, :, fam])
        u = y[:, :, fph] / np.abs(y[:, :, fph])
        cs = (u.real, u.imag)
        res = [np.matmul(np.transpose(u, (1, 3, 2, 0)), np.transpose(A, (1, 3, 0, 2)).astype(u.dtype)), A.sum(0),
               (A * A).sum(0), cs[0].sum(0), cs[1].sum(0), (cs[0] * cs[0]).sum(0), (cs[1] * cs[1]).sum(0),
               (cs[0] * cs[1]).sum(0)]
        t2 = time.perf_counter()
        del y, A, u, res
        say('(b) %s the host route: execute(cwt) to host %.1f ms + numpy formula %.1f ms = wall %.1f ms | host route / '
            'execute_erpac (%d epochs per chunk): wall %.0fx' % (dt, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3,
                                                                per_chunk, (t2 - t0) * 1e3 / min(wall[a])))
    plan.close()


say('# tools/erpac_rate.py on %s, %s' % (torch.cuda.get_device_name(0), os.environ.get('NINWAVE_LIB', 'libninwave.so')))
for dtype in ('float32', 'float64'):
    for per_chunk in (2, 8, 32):
        run(dtype, per_chunk, per_chunk == 32)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
