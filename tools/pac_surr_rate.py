"""Time-lag surrogate statistics of the coupling on device tensors (the library given by NINWAVE_LIB), NW_TIMING
plans, warm-up, the arms interleaved in one process, device time = the sum of the stage times of nw_plan_stats,
wall time around a synchronise.  No gate: what is measured is recorded (profiles/r23_pac_surr_rate.txt).

tools/pac_rate.py's shape: C = 8 channels, every channel with itself (P = 8), E = 64 epochs x n = 4096, F = 64
Morse scales of which the first 16 are the phase scales and the other 48 the amplitude scales, 128 signals per
chunk, fp32 and fp64, S = 200 lags drawn as pac_surrogates_batch draws them:
  (a) one Plan.execute_pac_surr call (M, amp, phase, stat) against one Plan.execute_pac call on the same plan: device,
      epilogue stage (the reduction kernels alone) and wall ms; the per-lag cost = (epilogue difference) / S, set
      against nw_pac_kernel alone (execute_pac without amp and phase), re-measured in the same run;
  (b) the host route the call replaces, execute(..., 'cwt') to host memory plus numpy per surrogate, at S = 8, one
      run, scaled to S = 200 (labelled as scaled);
  (c) the surrogate stage's rate, 4 E P nph nam T (S + 1) separately rounded fp64 operations, as a fraction of
      39.3e12 operations/s: half the 78.6 TFLOPS fp64 FMA figure of the specification (an FMA counts two, a
      separately rounded product or sum one); derived, not measured;
  (d) VGPRs, scratch and waves/SIMD of the kernels (tools/regs.py).
    python tools/pac_surr_rate.py [output file, default profiles/r23_pac_surr_rate.txt]"""
import os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import draw_lags

STAGES = ('ms_forward', 'ms_multiply', 'ms_inverse', 'ms_epilogue', 'ms_fused', 'ms_copy', 'ms_rows', 'ms_expand')
CEILING = 39.3e12
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'r23_pac_surr_rate.txt')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run(dt):
    n, E, C, F, batch, S = 4096, 64, 8, 64, 128, 200
    nph, nam = 16, 48
    fph, fam = np.arange(nph), np.arange(nph, nph + nam)
    tdt = torch.float32 if dt == 'float32' else torch.float64
    lags = draw_lags(n, S, seed=0)
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    tm = torch.empty((E, C, nph, nam), device='cuda', dtype=torch.complex128)
    ta = torch.empty((E, C, nam, 2), device='cuda', dtype=torch.float64)
    tu = torch.empty((E, C, nph), device='cuda', dtype=torch.complex128)
    ts = torch.empty((E, C, nph, nam, 4), device='cuda', dtype=torch.float64)

    def once(arm):
        if arm == 'surr':
            plan.execute_pac_surr(x, lags, None, fph, fam, out=(tm, ta, tu, ts))
        elif arm == 'surr/0':
            plan.execute_pac_surr(x, lags[:0], None, fph, fam, out=(tm, ta, tu, ts))
        elif arm == 'pac':
            plan.execute_pac(x, None, fph, fam, out=(tm, ta, tu))
        else:
            plan.execute_pac(x, None, fph, fam, out=(tm, None, None))

    arms = ('surr', 'surr/0', 'pac', 'pac/m')
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
    a, c = 'surr', 'pac'
    per_lag = (min(epi[a]) - min(epi[c])) / S
    say('(a) %s n=%d C=%d E=%d F=%d, %d phase x %d amplitude scales, P=%d own-channel pairs, S=%d lags: one execute_pac_surr: '
        'device %.3f ms (median %.3f), of it the reduction (epilogue stage, %d chunks) %.3f ms (median %.3f), wall %.3f ms '
        '(median %.3f) | one execute_pac: device %.3f ms (median %.3f), reduction %.3f ms (median %.3f), wall %.3f ms '
        '(median %.3f) | per lag (epilogue difference / S) %.4f ms | nw_pac_kernel alone (no amp / phase) %.3f ms '
        '(median %.3f): per lag / nw_pac_kernel alone %.3fx | execute_pac_surr with no lags (rows sums, staging, the lag 0): '
        'reduction %.3f ms (median %.3f)' % (
            dt, n, C, E, F, nph, nam, C, S, min(dev[a]), np.median(dev[a]), chunks, min(epi[a]), np.median(epi[a]),
            min(wall[a]), np.median(wall[a]), min(dev[c]), np.median(dev[c]), min(epi[c]), np.median(epi[c]), min(wall[c]),
            np.median(wall[c]), per_lag, min(epi['pac/m']), np.median(epi['pac/m']), per_lag / min(epi['pac/m']),
            min(epi['surr/0']), np.median(epi['surr/0'])))
    # (b) the host route at S = 8: every row over PCIe, then numpy per surrogate (one warm transform, one timed run)
    Sh = 8
    xh = x.cpu().numpy()
    plan.execute(xh.reshape(E * C, n), out_kind='cwt')
    t0 = time.perf_counter()
    y = plan.execute(xh.reshape(E * C, n), out_kind='cwt').reshape(E, C, F, n)
    t1 = time.perf_counter()
    A = np.abs(y[:, :, fam])
    u = y[:, :, fph] / np.abs(y[:, :, fph])
    h = [np.abs(np.matmul(u, np.swapaxes(np.roll(A, -int(l), axis=-1), -1, -2).astype(u.dtype))) for l in [0] + list(lags[:Sh])]
    res = [np.sum(h[1:], axis=0), np.sum(np.square(h[1:]), axis=0), np.sum([v >= h[0] for v in h[1:]], axis=0),
           np.max(h[1:], axis=0)]
    t2 = time.perf_counter()
    del y, A, u, h, res
    per = (t2 - t1) * 1e3 / (Sh + 1)
    scaled = (t1 - t0) * 1e3 + per * (S + 1)
    say('(b) %s the host route at S=%d: execute(cwt) to host %.1f ms + numpy %.1f ms (%.1f ms per surrogate) = wall %.1f ms; '
        'SCALED to S=%d: %.0f ms | scaled host route / execute_pac_surr: wall %.0fx' % (
            dt, Sh, (t1 - t0) * 1e3, (t2 - t1) * 1e3, per, (t2 - t0) * 1e3, S, scaled, scaled / min(wall[a])))
    plan.close()
    # (c) the surrogate stage against the fp64 vector rate for separately rounded operations
    ops = 4. * E * C * nph * nam * n * (S + 1)
    ms = min(epi[a])
    say('(c) %s the surrogate stage (rows sums, staging, %d lags): %.3f ms; 4 E P nph nam T (S + 1) = %.3e operations -> '
        '%.2fe12 operations/s = %.1f %% of 39.3e12 (derived from the specification, not measured; %.1f ms at that rate)' % (
            dt, S + 1, ms, ops, ops / (ms * 1e-3) / 1e12, 100 * ops / (ms * 1e-3) / CEILING, ops / CEILING * 1e3))


say('# tools/pac_surr_rate.py on %s, %s' % (torch.cuda.get_device_name(0), os.environ.get('NINWAVE_LIB', 'libninwave.so')))
run('float32')
run('float64')
# (d) the kernels' registers
for src in ('nw_pac_surr.hip', 'nw_pac.hip'):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'regs.py'), os.path.join(ROOT, 'ninwavelets_amd', 'csrc', src),
                        'kernel'], capture_output=True, text=True)
    for line in r.stdout.splitlines():
        say('(d) ' + line[:140])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
