"""Phase-binned phase-amplitude coupling on device tensors (the library given by NINWAVE_LIB), NW_TIMING plans,
warm-up, the arms interleaved in one process, device time = the sum of the stage times of nw_plan_stats, wall time
around a synchronise.  No gate: what is measured is recorded (profiles/r19_pac_bins_rate.txt).

The shape of tools/pac_rate.py: C = 8 channels, every channel with itself (P = 8), E = 64 epochs x n = 4096, F = 64
Morse scales of which the first 16 are the phase scales and the other 48 the amplitude scales, 128 signals per
chunk, nbins = 18, fp32 and fp64:
  (a) one Plan.execute_pac_bins call (S and count) against one Plan.execute_pac call (M, amp and phase) of the same
      plan: the same rows from the same transform stage -- device, epilogue stage (the reduction kernels alone)
      and wall ms;
  (b) against the host route the call replaces: execute(..., 'cwt') to host memory plus numpy (angle, digitize,
      hypot and one bincount per cell; wall, one run);
  (c) the reduction kernel alone (no counts) for nbins = 2, 18 and 36 (the three geometry classes) against what it
      does: the rows it reads once from HBM (C ec F n 2 esz per chunk) as a fraction of 8 TB/s, the hypots it forms
      and the LDS accumulator updates it makes, each per second.
With NINWAVE_LIB a diagnostic build (NW_ABL_PACBINS_NOHYPOT / _NOBIN / _NOLDS: wrong sums) the same lines show what
the kernel costs without its hypot, its edge tests or its LDS updates; such a run APPENDS its lines to the output
file, under its own header line naming the library, so that one file holds the product run and the A/B runs after it.
    python tools/pac_bins_rate.py [output file, default profiles/r19_pac_bins_rate.txt]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L

STAGES = ('ms_forward', 'ms_multiply', 'ms_inverse', 'ms_epilogue', 'ms_fused', 'ms_copy', 'ms_rows', 'ms_expand')
HBM = 8e12
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r19_pac_bins_rate.txt')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run(dt):
    n, E, C, F, batch = 4096, 64, 8, 64, 128
    nph, nam, nbins = 16, 48, 18
    fph, fam = np.arange(nph), np.arange(nph, nph + nam)
    esz = 4 if dt == 'float32' else 8
    tdt = torch.float32 if dt == 'float32' else torch.float64
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    tm = torch.empty((E, C, nph, nam), device='cuda', dtype=torch.complex128)
    ta = torch.empty((E, C, nam, 2), device='cuda', dtype=torch.float64)
    tu = torch.empty((E, C, nph), device='cuda', dtype=torch.complex128)
    ts = {nb: torch.empty((E, C, nph, nam, nb), device='cuda', dtype=torch.float64) for nb in (2, 18, 36)}
    tn = torch.empty((E, C, nph, nbins), device='cuda', dtype=torch.float64)

    def once(arm):
        if arm == 'pac':
            plan.execute_pac(x, None, fph, fam, out=(tm, ta, tu))
        elif arm == 'bins':
            plan.execute_pac_bins(x, None, fph, fam, nbins=nbins, out=(ts[nbins], tn))
        else:
            nb = int(arm.split('/')[1])
            plan.execute_pac_bins(x, None, fph, fam, nbins=nb, out=(ts[nb], None))

    arms = ('bins', 'pac', 'bins/2', 'bins/18', 'bins/36')
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
    a, c = 'bins', 'pac'
    say('(a) %s n=%d C=%d E=%d F=%d, %d phase x %d amplitude scales, P=%d own-channel pairs, nbins=%d: one execute_pac_bins: '
        'device %.3f ms (median %.3f), of it the reduction (epilogue stage, %d chunks) %.3f ms (median %.3f), wall %.3f ms '
        '(median %.3f) | one execute_pac: device %.3f ms (median %.3f), reduction %.3f ms (median %.3f), wall %.3f ms '
        '(median %.3f) | pac_bins / pac: device %.3fx reduction %.3fx wall %.3fx' % (
            dt, n, C, E, F, nph, nam, C, nbins, min(dev[a]), np.median(dev[a]), chunks, min(epi[a]), np.median(epi[a]),
            min(wall[a]), np.median(wall[a]), min(dev[c]), np.median(dev[c]), min(epi[c]), np.median(epi[c]), min(wall[c]),
            np.median(wall[c]), min(dev[a]) / min(dev[c]), min(epi[a]) / min(epi[c]), min(wall[a]) / min(wall[c])))
    # (b) the host route: every row over PCIe, then numpy (one warm transform, one timed run)
    xh = x.cpu().numpy()
    plan.execute(xh.reshape(E * C, n), out_kind='cwt')
    t0 = time.perf_counter()
    y = plan.execute(xh.reshape(E * C, n), out_kind='cwt').reshape(E, C, F, n)
    t1 = time.perf_counter()
    A = np.abs(y[:, :, fam])                                                       # (E, C, Fa, n)
    b = np.minimum(((np.angle(y[:, :, fph]) + np.pi) / (2 * np.pi / nbins)).astype(np.int64), nbins - 1)
    res = np.empty((E, C, nph, nam, nbins))
    for e in range(E):
        for ch in range(C):
            for i in range(nph):
                for k in range(nam):
                    res[e, ch, i, k] = np.bincount(b[e, ch, i], weights=A[e, ch, k], minlength=nbins)
    t2 = time.perf_counter()
    del y, A, b, res
    say('(b) %s the host route: execute(cwt) to host %.1f ms + numpy (angle, digitize, one bincount per cell) %.1f ms = '
        'wall %.1f ms | host route / execute_pac_bins: wall %.0fx' % (
            dt, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, (t2 - t0) * 1e3 / min(wall[a])))
    plan.close()
    # (c) the reduction kernel alone against what it does
    rows = E * C * F * n * 2 * esz
    values = E * C * nph * nam * n                                 # hypots, and LDS read-add-write updates
    for nb in (2, 18, 36):
        ms = min(epi['bins/%d' % nb])
        say('(c) %s nbins=%d nw_pac_bins_kernel alone: %.3f ms over %d launches (%.4f ms per epoch); the rows read once '
            '%.3f GB -> %.2f TB/s = %.1f %% of 8 TB/s; %.3g hypots and LDS updates -> %.1f G per second' % (
                dt, nb, ms, chunks, ms / E, rows / 1e9, rows / ms / 1e9, 100 * rows / (ms * 1e-3) / HBM, values,
                values / (ms * 1e-3) / 1e9))
    ms = min(epi['bins']) - min(epi['bins/18'])
    say('(c) %s nw_pac_bins_rows_kernel (the counts; epilogue with them - without): %.3f ms' % (dt, ms))


say('# tools/pac_bins_rate.py on %s, %s' % (torch.cuda.get_device_name(0), os.environ.get('NINWAVE_LIB', 'libninwave.so')))
run('float32')
run('float64')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'a' if os.environ.get('NINWAVE_LIB') else 'w') as f:
    f.write('\n'.join(lines) + '\n')
