"""Envelope correlation on device tensors (the library given by NINWAVE_LIB), NW_TIMING plans, warm-up, the arms
interleaved in one process, device time = the sum of the stage times of nw_plan_stats, wall time around a
synchronise, 50 calls per arm.  No gate: what is measured is recorded (profiles/r17_env_rate.txt).

C = 8 channels, all 28 pairs, E = 64 epochs x n = 4096, F = 64 Morse scales, 128 signals per chunk, fp32 and fp64:
  (a) one Plan.execute_env_time call in each mode (pair and per-channel sums) against one
      Plan.execute_conn_time(lag_sum) call on the same plan: the same rows from the same transform stage --
      device, epilogue stage (the reduction kernels alone) and wall ms;
  (b) against the host route the call replaces: execute(..., 'cwt') to host memory plus the numpy formula of
      the orthogonalised sums (wall, one run);
  (c) nw_env_time_kernel alone (no per-channel sums) against its algorithmic bytes -- the chunk's rows read
      once, C ec F n 2 esz -- as a fraction of 8 TB/s;
  (d) with --ablate LIB ...: the orthogonalised pair kernel alone under each diagnostic build of the library
      (make VARIANT=env_nodiv DEFS=-DNW_ABL_ENV_NODIV: the staging without hypot and divisions; VARIANT=env_noload
      DEFS=-DNW_ABL_ENV_NOLOAD: no global loads), one child process per library.
    python tools/env_rate.py [output file, default profiles/r17_env_rate.txt] [--ablate lib.so ...]"""
import os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import ninwavelets_amd as nw
from ninwavelets_amd import _lib as L
from ninwavelets_amd.engine import all_pairs

STAGES = ('ms_forward', 'ms_multiply', 'ms_inverse', 'ms_epilogue', 'ms_fused', 'ms_copy', 'ms_rows', 'ms_expand')
HBM = 8e12
ROUNDS = 50
args = sys.argv[1:]
child = bool(args) and args[0] == '--child'            # an ablation library: the pair kernel alone, to stdout
ablate = args[args.index('--ablate') + 1:] if '--ablate' in args else []
out_path = args[0] if args and not args[0].startswith('--') else os.path.join(ROOT, 'profiles', 'r17_env_rate.txt')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run(dt):
    n, E, C, F, batch = 4096, 64, 8, 64, 128
    esz = 4 if dt == 'float32' else 8
    tdt = torch.float32 if dt == 'float32' else torch.float64
    ia, ib = all_pairs(C)
    P = len(ia)
    plan = nw.Plan(n, F, dt, max_batch=batch, timing=True)
    plan.set_wavelet('morse', [17.5, 3.], np.arange(1., F + 1), L.trans_grid(n / 1000., 1000., False))
    common = torch.randn((E, 1, n), device='cuda', dtype=tdt)
    x = (0.6 * common + 0.8 * torch.randn((E, C, n), device='cuda', dtype=tdt)).contiguous()
    to = torch.empty((E, P, F, 6), device='cuda', dtype=torch.float64)
    tpl = torch.empty((E, P, F), device='cuda', dtype=torch.float64)
    tc = torch.empty((E, C, F, 2), device='cuda', dtype=torch.float64)
    tl = torch.empty((E, P, F, 4), device='cuda', dtype=torch.float64)

    def once(arm):
        if arm == 'orth':
            plan.execute_env_time(x, (ia, ib), out=(to, tc), out_kind='env_orth_sum')
        elif arm == 'orth/pair':
            plan.execute_env_time(x, (ia, ib), out=(to, None), out_kind='env_orth_sum')
        elif arm == 'plain':
            plan.execute_env_time(x, (ia, ib), out=(tpl, tc), out_kind='env_sum')
        elif arm == 'plain/pair':
            plan.execute_env_time(x, (ia, ib), out=(tpl, None), out_kind='env_sum')
        else:
            plan.execute_conn_time(x, (ia, ib), out=tl, out_kind='lag_sum')

    arms = ('orth/pair',) if child else ('orth', 'orth/pair', 'plain', 'plain/pair', 'lag')
    dev, epi, wall = ({k: [] for k in arms} for _ in range(3))
    for k in arms:
        once(k); plan.sync(); torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k in arms:
            plan.reset_stats()
            t0 = time.perf_counter(); once(k); plan.sync(); torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            st = plan.stats()
            dev[k].append(sum(st[s] for s in STAGES))
            epi[k].append(st['ms_epilogue'])
    chunks = st['chunks']
    if child:
        say('(d) %s %s: nw_env_time_kernel<orth> alone %.3f ms (median %.3f) over %d launches' % (
            dt, os.path.basename(os.environ.get('NINWAVE_LIB', 'libninwave.so')), min(epi['orth/pair']),
            np.median(epi['orth/pair']), chunks))
        plan.close()
        return
    head = '(a) %s n=%d C=%d E=%d F=%d, P=%d pairs, %d calls per arm:' % (dt, n, C, E, F, P, ROUNDS)
    for k, what in (('orth', 'one execute_env_time(env_orth_sum)'), ('plain', 'one execute_env_time(env_sum)'),
                    ('lag', 'one execute_conn_time(lag_sum)')):
        head += ' %s: device %.3f ms (median %.3f), of it the reduction (epilogue stage, %d chunks) %.3f ms (median %.3f), ' \
                'wall %.3f ms (median %.3f) |' % (what, min(dev[k]), np.median(dev[k]), chunks, min(epi[k]),
                                                  np.median(epi[k]), min(wall[k]), np.median(wall[k]))
    say(head + ' orth / lag: device %.3fx reduction %.3fx wall %.3fx | plain / lag: device %.3fx reduction %.3fx wall %.3fx' % (
        min(dev['orth']) / min(dev['lag']), min(epi['orth']) / min(epi['lag']), min(wall['orth']) / min(wall['lag']),
        min(dev['plain']) / min(dev['lag']), min(epi['plain']) / min(epi['lag']), min(wall['plain']) / min(wall['lag'])))
    # (b) the host route: every row over PCIe, then the numpy formula (one warm transform, one timed run)
    xh = x.cpu().numpy()
    plan.execute(xh.reshape(E * C, n), out_kind='cwt')
    t0 = time.perf_counter()
    y = plan.execute(xh.reshape(E * C, n), out_kind='cwt').reshape(E, C, F, n)
    t1 = time.perf_counter()
    res = []
    for ye in y:                                        # epoch by epoch: the (P, F, n) intermediates stay small
        A = np.abs(ye)
        w = ye / A
        a, b = w[ia], w[ib]
        q = np.abs(a.imag * b.real - a.real * b.imag)
        u, v = A[ia] * q, A[ib] * q
        res.append([u.sum(-1), (u * u).sum(-1), (u * A[ib]).sum(-1), v.sum(-1), (v * v).sum(-1), (v * A[ia]).sum(-1),
                    A.sum(-1), (A * A).sum(-1)])
    t2 = time.perf_counter()
    del y, A, w, a, b, q, u, v, res
    say('(b) %s the host route: execute(cwt) to host %.1f ms + numpy formula %.1f ms = wall %.1f ms | host route / '
        'execute_env_time(env_orth_sum): wall %.0fx' % (dt, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3,
                                                        (t2 - t0) * 1e3 / min(wall['orth'])))
    plan.close()
    # (c) the pair kernel against the rows read once
    rows = E * C * F * n * 2 * esz
    for k, what in (('orth/pair', 'nw_env_time_kernel<orth> alone'), ('plain/pair', 'nw_env_time_kernel<plain> alone'),
                    ('orth', 'nw_env_time_kernel<orth> + nw_env_chan_kernel')):
        ms = min(epi[k])
        say('(c) %s %s: %.3f ms over %d launches (%.4f ms per epoch); the rows read once %.3f GB -> %.2f TB/s = %.1f %% of '
            '8 TB/s' % (dt, what, ms, chunks, ms / E, rows / 1e9, rows / ms / 1e9, 100 * rows / (ms * 1e-3) / HBM))


if child:
    run('float32')
    run('float64')
    sys.exit(0)
say('# tools/env_rate.py on %s, %s' % (torch.cuda.get_device_name(0), os.environ.get('NINWAVE_LIB', 'libninwave.so')))
run('float32')
run('float64')
for lib in ablate:                                      # (d): a fresh process per diagnostic library
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, NINWAVE_LIB=os.path.abspath(lib)))
    if r.returncode != 0:
        say('(d) %s: exit %d: %s' % (lib, r.returncode, r.stderr[-300:]))
        break
    for ln in r.stdout.splitlines():
        if ln.startswith('(d)'):
            say(ln)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
