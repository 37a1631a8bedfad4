"""GPU tests of the cross-channel pair reductions: nw_execute_pair (k_accumulate_pair over the
chunk's complex rows, nw_kernels.hip; fp64 block partials inside nw_fused_pair_kernel where
nw_pair_partials_supported, nw_fused.hip) through Plan.execute_pair, WaveletBase.cross_batch and
EpochsWavelet.csd / coherence / imcoh / plv.

For epochs e, channel rows y_a,e and y_b,e (F, n_out):
    S_ab = sum_e y_a conj(y_b),  P_aa = sum_e |y_a|^2,  Phi_ab = sum_e (y_a/|y_a|) conj(y_b/|y_b|)
every sum in fp64 in epoch order.  References are formed here from oracle.nw_oracle in complex128.

Inputs: pair_rows of epoch_cases.py: rng = default_rng(2100 + n), a = rng.standard_normal((E, n)), b = 0.6 a + 0.8 rng.standard_normal((E, n)),
Morse(1000) with its default b, r, nine scales (one more than a tile), E = 6 epochs (12 signals: two
blocks of 8, the second holding 2 pairs).

Bounds.  A_e, B_e: each reference signal's max|y| over (F, N); tol: the project's per-signal
tolerance, 1e-12 fp64, 1e-5 fp32, 2e-5 fp32 on chirp-z lengths (test_gpu_chirp.py).
  T1  |dS_ab| <= 2 tol sum_e A_e B_e,  |dP_aa| <= 2 tol sum_e A_e^2  (pointwise, against the oracle)
  T2  against the same plan's own rows reduced in numpy complex128: 1e-13 sum_e |y_a||y_b| (the
      project's bound for the same fp64 additions of the same values, regrouped), 1e-13 E for Phi
  T3  v = 0.01: |dplv| <= 2 tol / v where every epoch has |y_a| >= v A_e, |y_b| >= v B_e (a phasor
      of a value known to tol A at magnitude >= v A is off by <= tol / v; two phasors per product);
      fp64 |dcoherence| <= 4 tol / v^2 where P_aa >= v^2 sum A_e^2 and P_bb >= v^2 sum B_e^2
Measured maxima (MI355X), as fractions of the bounds: see DESIGN.md section 5."""
import numpy as np
import pytest

from epoch_cases import FREQS, FREQS3, FakeEpochs, forms, morse_plan, tol_of
from epoch_cases import pair_rows as oracle_rows

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402
from ninwavelets_amd.engine import finalize_pair  # noqa: E402

E6 = 6
V = 0.01
DTYPES = ['float32', 'float64']
OUTS = ['cross_sum', 'plv_sum', 'csd', 'coherency', 'coherence', 'imcoh', 'plv']


def sums_of(ya, yb):
    """(cross (F, n, 4), phi (F, n)) of complex128 rows (E, F, n), added in epoch order."""
    s = np.zeros(ya.shape[1:], dtype=np.complex128)
    paa = np.zeros(ya.shape[1:])
    pbb = np.zeros(ya.shape[1:])
    phi = np.zeros(ya.shape[1:], dtype=np.complex128)
    with np.errstate(invalid='ignore', divide='ignore'):
        for e in range(ya.shape[0]):
            s += ya[e] * np.conj(yb[e])
            paa += np.abs(ya[e]) ** 2
            pbb += np.abs(yb[e]) ** 2
            phi += (ya[e] / np.abs(ya[e])) * np.conj(yb[e] / np.abs(yb[e]))
    return np.stack([s.real, s.imag, paa, pbb], axis=-1), phi


# (id, n, dtype, E, freqs, plan keywords, decim, kernel of the form): every size the fused pair partials may cover,
# in both dtypes, then the other forms; six epochs of the nine scales but for the two-pass row
CASES = [(f'pair-{n}', n, 'float32', E6, FREQS, {}, 1, 'nw_fused_pair_kernel') for n in (1024, 2048, 4096)]
CASES += [(f'f64-{n}', n, 'float64', E6, FREQS, {}, 1, 'nw_fused_kernel') for n in (1024, 2048, 4096)]
for name, n, dtype, kw, decim, _, kernel in forms('e32-8192', 'chirp-1201-f32', 'chirp-1201-f64', 'rocfft-1000',
                                                  'twopass-32768', 'decim-4096'):
    E, freqs = (3, FREQS3) if name == 'twopass-32768' else (E6, FREQS)
    CASES.append((name, n, dtype, E, freqs, kw, decim, kernel))


def cross_err(got, ya, yb):
    """max over points of |got - ref| / scale for S_ab, P_aa, P_bb, with T1's per-signal scales
    sum_e A_e B_e, sum_e A_e^2, sum_e B_e^2."""
    want, _ = sums_of(ya, yb)
    A = np.max(np.abs(ya), axis=(1, 2))
    B = np.max(np.abs(yb), axis=(1, 2))
    ds = np.abs((got[..., 0] + 1j * got[..., 1]) - (want[..., 0] + 1j * want[..., 1]))
    return (np.max(ds) / np.sum(A * B), np.max(np.abs(got[..., 2] - want[..., 2])) / np.sum(A * A),
            np.max(np.abs(got[..., 3] - want[..., 3])) / np.sum(B * B))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_cross_sums_against_the_oracle_and_the_plans_own_rows(case):
    """T1 and T2 on one plan per case."""
    name, n, dtype, E, freqs, kw, decim, kernel = case
    a, b, ya, yb = oracle_rows(n, E, dtype, freqs)
    ya, yb = ya[..., ::decim], yb[..., ::decim]
    tol = tol_of(n, dtype)
    p = morse_plan(n, dtype, freqs, 2 * E, decim=decim, **kw)
    try:
        cross = p.execute_pair(a, b, out_kind='cross_sum')
        st = p.stats()
        path_cross = st['reduce_path']
        phi = p.execute_pair(a, b, out_kind='plv_sum')
        path_plv = p.stats()['reduce_path']
        inter = np.empty((2 * E, n), dtype=dtype)
        inter[0::2], inter[1::2] = a, b
        rows = p.execute(inter, out_kind='cwt').astype(np.complex128)
    finally:
        p.close()
    assert cross.shape == (len(freqs), n // decim, 4) and cross.dtype == np.float64
    assert phi.shape == (len(freqs), n // decim) and phi.dtype == np.complex128
    assert L.KERNEL_NAMES[st['kernel']] == kernel, st
    f32 = L.NW_F32 if dtype == 'float32' else L.NW_F64
    fusable = decim == 1 and not kw
    for path, ok in ((path_cross, L.NW_OUT_CROSS_SUM), (path_plv, L.NW_OUT_PLV_SUM)):
        want_path = 2 if fusable and L.pair_partials_supported(n, f32, L.NW_MORSE, ok) else 1
        assert path == want_path, (name, ok, path)
    # T1
    es, ea, eb = cross_err(cross, ya, yb)
    print(f'{name} T1: dS {es / (2 * tol):.3f} dPaa {ea / (2 * tol):.3f} dPbb {eb / (2 * tol):.3f} of the bound (tol {tol:.0e})')
    assert es <= 2 * tol and ea <= 2 * tol and eb <= 2 * tol, (name, es, ea, eb)
    # T2
    ra, rb = rows[0::2], rows[1::2]
    own, own_phi = sums_of(ra, rb)
    sab = np.sum(np.abs(ra) * np.abs(rb), axis=0)
    ds = np.abs((cross[..., 0] + 1j * cross[..., 1]) - (own[..., 0] + 1j * own[..., 1]))
    da = np.abs(cross[..., 2] - own[..., 2])
    db = np.abs(cross[..., 3] - own[..., 3])
    paa, pbb = np.sum(np.abs(ra) ** 2, axis=0), np.sum(np.abs(rb) ** 2, axis=0)
    pos = np.all(np.abs(ra) > 0, axis=0) & np.all(np.abs(rb) > 0, axis=0)
    dphi = np.abs(phi - own_phi)[pos]
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = [np.nanmax(np.where(sab > 0, ds / sab, 0)), np.nanmax(np.where(paa > 0, da / paa, 0)),
                 np.nanmax(np.where(pbb > 0, db / pbb, 0)), np.max(dphi) / E]
    print(f'{name} T2: dS {worst[0]:.2e} dPaa {worst[1]:.2e} dPbb {worst[2]:.2e} dPhi/E {worst[3]:.2e} (bound 1e-13); '
          f'{pos.mean():.3f} of the points have every |y| > 0')
    assert np.all(ds <= 1e-13 * sab) and np.all(da <= 1e-13 * paa) and np.all(db <= 1e-13 * pbb), (name, worst)
    assert pos.mean() >= 0.5 and np.all(dphi <= 1e-13 * E), (name, worst)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [1024, 1201])
def test_plv_and_coherence_on_visible_points(n, dtype):
    """T3."""
    a, b, ya, yb = oracle_rows(n, E6, dtype, FREQS)
    tol = tol_of(n, dtype)
    A = np.max(np.abs(ya), axis=(1, 2))[:, None, None]
    B = np.max(np.abs(yb), axis=(1, 2))[:, None, None]
    vis = np.all(np.abs(ya) >= V * A, axis=0) & np.all(np.abs(yb) >= V * B, axis=0)
    per_row = vis.mean(axis=1)
    assert np.all(per_row >= 0.5), per_row                 # on the reference alone
    want_cross, want_phi = sums_of(ya, yb)
    p = morse_plan(n, dtype, FREQS, 2 * E6)
    try:
        cross = p.execute_pair(a, b, out_kind='cross_sum')
        phi = p.execute_pair(a, b, out_kind='plv_sum')
    finally:
        p.close()
    dplv = np.abs(finalize_pair('plv', phi, E6) - finalize_pair('plv', want_phi, E6))
    worst = np.max(dplv[vis])
    print(f'n={n} {dtype} T3: visible {per_row.min():.2f}-{per_row.max():.2f} per row, {vis.mean():.2f} overall; '
          f'dplv {worst:.3e} = {worst / (2 * tol / V):.4f} of the bound')
    assert worst <= 2 * tol / V
    if dtype == 'float64':
        pvis = (want_cross[..., 2] >= V * V * np.sum(A * A)) & (want_cross[..., 3] >= V * V * np.sum(B * B))
        assert pvis.mean() >= 0.9, pvis.mean()
        dcoh = np.abs(finalize_pair('coherence', cross, E6) - finalize_pair('coherence', want_cross, E6))
        print(f'n={n} {dtype} T3: power-visible {pvis.mean():.3f}; dcoherence {np.max(dcoh[pvis]):.3e} = '
              f'{np.max(dcoh[pvis]) / (4 * tol / V ** 2):.2e} of the bound')
        assert np.max(dcoh[pvis]) <= 4 * tol / V ** 2


@pytest.mark.parametrize('dtype', DTYPES)
def test_chunking_changes_nothing_but_the_grouping(dtype):
    """T4: max_batch 12 (one chunk), 5 and 4 (chunks of 2 pairs), 2 (one pair per chunk)."""
    n = 2048
    a, b, ya, yb = oracle_rows(n, E6, dtype, FREQS)
    sab = np.sum(np.abs(ya) * np.abs(yb), axis=0)
    paa, pbb = np.sum(np.abs(ya) ** 2, axis=0), np.sum(np.abs(yb) ** 2, axis=0)
    got = {}
    for mb in (12, 5, 4, 2):
        p = morse_plan(n, dtype, FREQS, mb)
        try:
            got[mb] = (p.execute_pair(a, b, out_kind='cross_sum'), p.execute_pair(a, b, out_kind='plv_sum'))
            assert p.stats()['chunks'] == 2 * -(-E6 // (mb // 2)), (mb, p.stats())
        finally:
            p.close()
    for mb in (5, 4, 2):
        c, c0 = got[mb][0], got[12][0]
        ds = np.abs((c[..., 0] + 1j * c[..., 1]) - (c0[..., 0] + 1j * c0[..., 1]))
        dphi = np.abs(got[mb][1] - got[12][1])
        print(f'{dtype} max_batch {mb}: dS {np.max(ds / sab):.2e} dPhi/E {np.max(dphi) / E6:.2e}')
        assert np.all(ds <= 1e-13 * sab)
        assert np.all(np.abs(c[..., 2] - c0[..., 2]) <= 1e-13 * paa) and np.all(np.abs(c[..., 3] - c0[..., 3]) <= 1e-13 * pbb)
        assert np.all(dphi <= 1e-13 * E6)
    p = morse_plan(n, dtype, FREQS, 1)
    try:
        with pytest.raises(ValueError, match='max_batch'):
            p.execute_pair(a, b)
        assert p.execute(a[:1], out_kind='power').shape == (1, len(FREQS), n)      # the plan still works
    finally:
        p.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_epoch_and_no_pairs(dtype):
    """T5: epoch 2 of channel b all zero: its rows are exactly 0, so Phi is NaN at every point
    (0/0, as ITC) while S_ab, P_aa, P_bb are the sums the oracle gives (that epoch adds 0 to S_ab
    and P_bb); npairs = 0 gives zero sums."""
    n = 1024
    a, b, ya, yb = oracle_rows(n, E6, dtype, FREQS, zero_b=2)
    assert not np.any(b[2]) and not np.any(yb[2])
    tol = tol_of(n, dtype)
    p = morse_plan(n, dtype, FREQS, 2 * E6)
    try:
        cross = p.execute_pair(a, b, out_kind='cross_sum')
        phi = p.execute_pair(a, b, out_kind='plv_sum')
        none_c = p.execute_pair(a[:0], b[:0], out_kind='cross_sum')
        none_p = p.execute_pair(a[:0], b[:0], out_kind='plv_sum')
    finally:
        p.close()
    assert np.all(np.isnan(phi.real)) and np.all(np.isnan(phi.imag))
    assert np.all(np.isfinite(cross))
    es, ea, eb = cross_err(cross, ya, yb)
    assert es <= 2 * tol and ea <= 2 * tol and eb <= 2 * tol, (es, ea, eb)
    assert np.all(np.isfinite(finalize_pair('coherence', cross, E6)))
    assert none_c.shape == cross.shape and not np.any(none_c)
    assert none_p.shape == phi.shape and not np.any(none_p)


@pytest.mark.parametrize('dtype', DTYPES)
def test_device_tensors_equal_the_host_call_bit_for_bit(dtype):
    """T6: torch inputs and outputs, ordered with torch's current stream; the same fp64 additions
    in the same order as the host-array call."""
    import torch
    n = 1024
    a, b, _, _ = oracle_rows(n, E6, dtype, FREQS)
    p = morse_plan(n, dtype, FREQS, 8)                    # chunks of 4 and 2 pairs
    try:
        host = (p.execute_pair(a, b, out_kind='cross_sum'), p.execute_pair(a, b, out_kind='plv_sum'))
        ta = torch.from_numpy(np.array(a)).cuda()
        tb = torch.from_numpy(np.array(b)).cuda()
        oc = torch.full((len(FREQS), n, 4), float('nan'), dtype=torch.float64, device='cuda')
        op = torch.full((len(FREQS), n), float('nan'), dtype=torch.complex128, device='cuda')
        assert p.execute_pair(ta, tb, out=oc, out_kind='cross_sum') is oc
        p.execute_pair(ta, tb, out=op, out_kind='plv_sum')
        dev = (oc.cpu().numpy(), op.cpu().numpy())
        with pytest.raises(ValueError, match='output'):
            p.execute_pair(ta, tb, out_kind='cross_sum')
        with pytest.raises(ValueError, match='float64'):
            p.execute_pair(ta, tb, out=op, out_kind='cross_sum')
        with pytest.raises(ValueError, match='same number'):
            p.execute_pair(ta, tb[:3], out=oc, out_kind='cross_sum')
    finally:
        p.close()
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_class_api(dtype):
    """T7: Morse.cross_batch for every out and EpochsWavelet.csd / coherence / imcoh / plv against
    numpy on the oracle sums (T1 / T3 bounds), and the finalised outputs against finalize_pair of
    the same call's sums (exactly: the sums are deterministic)."""
    n = 1024
    a, b, ya, yb = oracle_rows(n, E6, dtype, FREQS)
    tol = tol_of(n, dtype)
    want_cross, want_phi = sums_of(ya, yb)
    A = np.max(np.abs(ya), axis=(1, 2))[:, None, None]
    B = np.max(np.abs(yb), axis=(1, 2))[:, None, None]
    vis = np.all(np.abs(ya) >= V * A, axis=0) & np.all(np.abs(yb) >= V * B, axis=0)
    w = nw.Morse(1000, dtype=dtype)
    got = {out: w.cross_batch(a, b, FREQS, out=out) for out in OUTS}
    assert len(w._plans) == 1
    assert got['cross_sum'].shape == (len(FREQS), n, 4) and got['cross_sum'].dtype == np.float64
    es, ea, eb = cross_err(got['cross_sum'], ya, yb)
    assert es <= 2 * tol and ea <= 2 * tol and eb <= 2 * tol, (es, ea, eb)
    assert np.max(np.abs(got['csd'] - finalize_pair('csd', want_cross, E6))) <= 2 * tol * np.sum(A * B) / E6
    assert np.max(np.abs(got['plv'] - finalize_pair('plv', want_phi, E6))[vis]) <= 2 * tol / V
    for out in OUTS:
        src = got['plv_sum'] if out in ('plv', 'plv_sum') else got['cross_sum']
        assert np.array_equal(got[out], finalize_pair(out, src, E6)), out
        assert got[out].dtype == (np.complex128 if out in ('plv_sum', 'csd', 'coherency') else np.float64), out
    if dtype == 'float64':
        pvis = (want_cross[..., 2] >= V * V * np.sum(A * A)) & (want_cross[..., 3] >= V * V * np.sum(B * B))
        assert pvis.mean() >= 0.9
        for out in ('coherency', 'coherence', 'imcoh'):
            assert np.max(np.abs(got[out] - finalize_pair(out, want_cross, E6))[pvis]) <= 4 * tol / V ** 2, out
    assert np.all(got['coherence'] <= 1 + 1e-12) and np.all(got['plv'][vis] <= 1 + 1e-12)
    # (..., N) inputs are flattened to pairs
    assert np.array_equal(w.cross_batch(a.reshape(2, 3, n), b.reshape(2, 3, n), out='cross_sum'), got['cross_sum'])
    # EpochsWavelet: channels of one (epochs, channels, samples) array
    data = np.stack([a, b, a], axis=1)
    ew = nw.EpochsWavelet(FakeEpochs(data, 1000., ['a', 'b', 'c']), nw.Morse(1000, dtype=dtype))
    for out in ('csd', 'coherence', 'imcoh', 'plv'):
        assert np.array_equal(getattr(ew, out)('a', 'b', FREQS), got[out]), out
    assert np.max(np.abs(ew.coherence('a', 'c', FREQS) - 1)) <= 1e-15
    # decim: on the device where supported (n = 4096, decim 4), else sliced from the full sums
    a4, b4, ya4, yb4 = oracle_rows(4096, E6, dtype, FREQS)
    w4 = nw.Morse(1000, dtype=dtype)
    c4 = w4.cross_batch(a4, b4, FREQS, out='cross_sum', decim=4)
    assert c4.shape == (len(FREQS), 1024, 4)
    assert L.KERNEL_NAMES[w4.plan_stats()[0]['kernel']] == 'nw_fused_decim_kernel'
    assert max(cross_err(c4, ya4[..., ::4], yb4[..., ::4])) <= 2 * tol_of(4096, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_decim_fallback_is_the_sliced_result(dtype):
    """T7: n = 1201 has no device decimation: decim = 5 is the undecimated result [..., ::5], exactly."""
    n = 1201
    a, b, _, _ = oracle_rows(n, E6, dtype, FREQS)
    w = nw.Morse(1000, dtype=dtype)
    for out in OUTS:
        full = w.cross_batch(a, b, FREQS, out=out)
        dec = w.cross_batch(a, b, FREQS, out=out, decim=5)
        sl = full[:, ::5]
        assert dec.shape == sl.shape and np.array_equal(dec, sl, equal_nan=True), out
    assert len(w._plans) == 1
