"""GPU parity of the two-pass form (nw_large.hip, n = 2^15 .. 2^24) at every (N1, N2) split with
every epilogue, and of its row pass with every pruned pass-0 variant idft_br<T, E, NZ>, four rows
per workgroup and one, analytic and complex table rows, in both dtypes.

Which kernels a case runs is restated in tests/large_variants.py; which variant a row takes is
read from the plan itself: Plan.row_support() is km, the bound rows_kernel prunes to, and
need() / variant() of the helper at the first and last row k1 give the NZ.  The variant sets are
asserted: a case that misses one fails.  Every run asserts the fused engine, row-pass launches,
the kernel cols_kernel and row_support(scan=True) == row_support().

Signals are white noise drawn as float32 and handed to both dtypes.  References in complex128:
oracle.nw_oracle.cwt for the stock kinds, cwt_from_rows on the exact rows handed to the plan for
tables; |.| and |.|^2 are taken from them.  Tolerance, per (signal, row): max|got_row - ref_row|
<= tol x max|ref_row| with tol = large_variants.tol_f32(n) for fp32 (1e-5 to 2^16, 3e-5 above) and
1e-12 for fp64, doubled for power.

The row pass gives a workgroup kRowGroup = 4 rows when a launch holds >= 8 scales, else one:
cases 2 - 5 run F = 9 scales whole (grouped) and again in launches of 3 scales (NW_LARGE_FCHUNK=3,
one row per workgroup) and require the two outputs to be equal bit for bit, since the arithmetic
of a row does not depend on how rows are grouped."""
import numpy as np
import pytest

import large_variants as V
from oracle import nw_oracle as O

pytestmark = pytest.mark.gpu

import ninwavelets_amd as nw  # noqa: E402
from ninwavelets_amd import _lib as L  # noqa: E402

SFREQ = 1000.
DTYPES = ['float32', 'float64']
ROW_SIZES = [1 << e for e in range(15, 20)]          # N1 = 32, N2 = 1024 .. 16384
MAXIMA = {}                                           # (dtype, out) -> largest error / max|ref_row| seen


def tol(dtype, n, out='cwt'):
    return (V.tol_f32(n) if dtype == 'float32' else 1e-12) * (2 if out == 'power' else 1)


def noise(S, n, seed):
    return np.random.default_rng(seed).standard_normal((S, n)).astype(np.float32)


_cache = {}


def cached(slot, key, make):
    """One reference per slot at a time (the dtype varies fastest, so both dtypes share it)."""
    hit = _cache.get(slot)
    if hit is None or hit[0] != key:
        _cache[slot] = hit = (key, make())
    return hit[1]


def as_kind(c, out):
    return c if out == 'cwt' else np.abs(c) if out == 'abs' else np.abs(c) ** 2


def check_rows(got, ref, t, dtype, out, what):
    """Per (signal, row): max|got - ref| <= t x max|ref|."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.max(np.abs(got - ref), axis=-1) / np.max(np.abs(ref), axis=-1)
    worst = float(np.max(err))
    MAXIMA[dtype, out] = max(MAXIMA.get((dtype, out), 0.0), worst)
    print(f'{what} {dtype} {out}: max row error {worst:.3e} (tol {t:.0e}); '
          f'largest so far {dtype} {out} {MAXIMA[dtype, out]:.3e}')
    assert np.all(err <= t), (what, dtype, out, err)


def stock(kind):
    return (nw.Morse(SFREQ) if kind == 'morse' else nw.Morlet(SFREQ))._analytic()


def attach_stock(kind, n, freqs):
    name, params = stock(kind)
    grid = L.trans_grid(n / SFREQ, SFREQ, False)
    return lambda p: p.set_wavelet(name, params, np.asarray(freqs, dtype=np.float64), grid)


def attach_table(table):
    F, n = table.shape
    return lambda p: p.set_wavelet('table', [], np.arange(1., F + 1), L.nw_grid(1.0, n, n), table=table)


def support(n, dtype, kind, freqs):
    """km of every scale of ``freqs`` from a plan of its own (nothing is executed)."""
    p = nw.Plan(n, len(freqs), dtype)
    try:
        attach_stock(kind, n, freqs)(p)
        return p.row_support().astype(np.int64)
    finally:
        p.close()


def run(n, dtype, F, attach, x, outs=('cwt',), chunk=None):
    """One plan, every out kind of ``outs``; -> (results, km).  ``chunk``: the scales per launch
    pair the caller set with NW_LARGE_FCHUNK (None: one launch pair holds them all)."""
    S = x.shape[0]
    launches = S * (-(-F // chunk) if chunk else 1)
    p = nw.Plan(n, F, dtype, max_batch=S)
    try:
        attach(p)
        km = p.row_support().astype(np.int64)
        np.testing.assert_array_equal(p.row_support(scan=True), km)
        got = {}
        for i, out in enumerate(outs):
            got[out] = p.execute(x, out_kind=out)
            st = p.stats()
            assert st['engine'] == 'fused' and L.KERNEL_NAMES[st['kernel']] == 'cols_kernel', st
            assert st['launches_rows'] == (i + 1) * launches > 0, (st, launches)
            assert st['unique_rows'] == F, st
    finally:
        p.close()
    return got, km


def whole_and_chunked(n, dtype, F, attach, x, ref, what, monkeypatch):
    """F scales in one launch pair (four rows per workgroup) and in launches of 3 (one row per
    workgroup): both against the reference, and equal bit for bit.  -> km."""
    assert V.row_group(F) == 4 and V.row_group(3) == 1 and F % 8
    whole, km = run(n, dtype, F, attach, x)
    monkeypatch.setenv('NW_LARGE_FCHUNK', '3')
    chunked, km3 = run(n, dtype, F, attach, x, chunk=3)
    monkeypatch.delenv('NW_LARGE_FCHUNK')
    np.testing.assert_array_equal(km3, km)
    check_rows(whole['cwt'], ref, tol(dtype, n), dtype, 'cwt', what + ' grouped')
    check_rows(chunked['cwt'], ref, tol(dtype, n), dtype, 'cwt', what + ' one row per workgroup')
    np.testing.assert_array_equal(whole['cwt'], chunked['cwt'])
    print(f'{what} {dtype}: grouped == one row per workgroup, bit for bit')
    return km


def geometry(n, dtype, table):
    n1, n2 = V.split(n)
    e = V.row_elems(n2, dtype, table)
    return n1, n2, e, n2 // e, V.ladder(e, dtype, table)


def row_variants(km, n1, t, lad):
    """(NZ at k1 = 0, NZ at k1 = N1 - 1) of a row with support bound km."""
    return V.variant(V.need(km, 0, n1, t), lad), V.variant(V.need(km, n1 - 1, n1, t), lad)


# ------------------------------------------------------------------ 1. every split, every epilogue
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [1 << e for e in range(15, 24)])
def test_every_split_every_epilogue(n, dtype):
    """Every (N1, N2) of cols_t below 2^24 (N1 = 32 with N2 = 1024 .. 16384, then N2 = 16384 with
    N1 = 64 .. 512; n = 2^23 is the smallest shape with N1 = 512) x {cwt, abs, power}: Morse at
    3, 60 and 250 Hz, one signal, against the oracle."""
    freqs = [3., 60., 250.]
    x = noise(1, n, 1000 + n % 977)
    ref = cached('split', n, lambda: O.cwt('morse', x[0].astype(np.float64), freqs))
    got, km = run(n, dtype, 3, attach_stock('morse', n, freqs), x, outs=('cwt', 'abs', 'power'))
    print(f'n=2^{n.bit_length() - 1} split {V.split(n)} km {km.tolist()}')
    for out in ('cwt', 'abs', 'power'):
        check_rows(got[out][0], as_kind(ref, out), tol(dtype, n, out), dtype, out, f'split n=2^{n.bit_length() - 1}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_c5_length_abs_and_power_epilogues(dtype):
    """N1 = 1024 (n = 2^24): the |y| and |y|^2 epilogues against |cwt| and |cwt|^2 of the same
    plan's cwt output, which test_gpu_parity.py::test_c5_scale_single_signal holds to the oracle;
    its bounds (1e-4 fp32, 1e-12 fp64; doubled for power), per row."""
    n = 1 << 24
    assert V.split(n) == (1024, 16384)
    freqs = [60., 250.]
    t = 1e-4 if dtype == 'float32' else 1e-12
    got, _ = run(n, dtype, 2, attach_stock('morse', n, freqs), noise(1, n, 24), outs=('cwt', 'abs', 'power'))
    c = got['cwt'][0].astype(np.complex128)
    assert np.all(np.max(np.abs(c), axis=-1) > 0)
    check_rows(got['abs'][0], np.abs(c), t, dtype, 'abs', 'n=2^24 vs own cwt')
    check_rows(got['power'][0], np.abs(c) ** 2, 2 * t, dtype, 'power', 'n=2^24 vs own cwt')


# ------------------------------------------------------------------ table rows
def make_rows(supports, n, seed, lift=()):
    """(F, n) complex128: row i is complex normal on [0, supports[i]) / sqrt(supports[i]) and
    exactly zero from there on (tests/test_gpu_table_rows.py).  Rows listed in ``lift`` get their
    two last bins scaled up to a sixth of the other bins' energy each, a quarter of the row's
    energy together."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((len(supports), n), dtype=np.complex128)
    for i, k in enumerate(supports):
        tab[i, :k] = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) / np.sqrt(k)
        if i in lift:
            rest = np.sum(np.abs(tab[i, :k - 2]) ** 2)
            last = tab[i, k - 2:k]
            tab[i, k - 2:k] = last / np.abs(last) * np.sqrt(rest / 6)
    assert len({r.tobytes() for r in tab}) == len(supports)            # no repeated rows
    return tab


def table_case(slot, n, supports, x, seed, lift=()):
    """(table, reference) of the rows with ``supports``: cwt_from_rows on the table's own rows."""
    def make():
        table = make_rows(supports, n, seed, lift)
        return table, np.stack([O.cwt_from_rows(xi.astype(np.float64), list(table), False) for xi in x])
    return cached(slot, (n, tuple(supports)), make)


def more_needs(needs, e, have=0):
    """Further needs, none of ``needs``, until the plan (``have`` other rows + needs + these) holds
    F >= 9 scales and F is no multiple of the 8-scale tile."""
    extra = [nd for nd in (2, 6, 12, 14, 20, 28, 10, 30) if nd <= e and nd not in needs]
    more = []
    while have + len(needs) + len(more) < 9 or (have + len(needs) + len(more)) % 8 == 0:
        more.append(extra.pop(0))
    return more


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', ROW_SIZES)
def test_table_rows_every_variant_grouped_and_ungrouped(n, dtype, monkeypatch):
    """Complex table rows (KIND == NW_TABLE: fp32 E = 16 / 32, fp64 E = 16 at every N2) with hard
    supports [0, K): one row per need in {1, 3} + ladder at the middle of its element,
    K = (2 need - 1) (n / E) / 2, and further needs up to F = 9.  km == K - 1 and the set of
    variants hit == the ladder are asserted from the plan."""
    n1, n2, e, t, lad = geometry(n, dtype, True)
    bins = n // e                                                       # bins per pass-0 element
    needs = [1, 3] + sorted(lad)
    needs += more_needs(needs, e)
    supports = [(2 * nd - 1) * bins // 2 for nd in needs]
    F = len(supports)
    x = noise(2, n, 2000 + n % 977)
    table, ref = table_case('table', n, supports, x, 2100 + n % 977)
    km = whole_and_chunked(n, dtype, F, attach_table(table), x, ref, f'table variants n=2^{n.bit_length() - 1}',
                           monkeypatch)
    np.testing.assert_array_equal(km, np.array(supports) - 1)
    nz = [row_variants(k, n1, t, lad) for k in km]
    assert all(a == b for a, b in nz), nz
    assert [V.need(k, 0, n1, t) for k in km] == needs
    hit = {a for a, _ in nz}
    assert hit == lad, f'row variants hit {sorted(hit)} != ladder {sorted(lad)}'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', ROW_SIZES)
def test_table_rows_need_changes_inside_a_group(n, dtype, monkeypatch):
    """need_of(k1) drops by one at k1 = km mod (n / E) + 1.  For every q of the ladder below E, rows
    with K = q (n / E) + 2 and + 6: km mod (n / E) is 1 and 5, so the four-row workgroup of rows
    0 .. 3 and that of rows 4 .. 7 each run two variants back to back.  The two last bins of such
    a row carry a quarter of its energy, so a row computed with one element too few is wrong by
    far more than the tolerance."""
    n1, n2, e, t, lad = geometry(n, dtype, True)
    bins = n // e
    steps = [(q, off) for q in sorted(v for v in lad if v < e) for off in (2, 6)]
    supports = [q * bins + off for q, off in steps]
    supports += [(2 * nd - 1) * bins // 2 for nd in more_needs([], e, have=len(steps))]
    F = len(supports)
    x = noise(2, n, 3000 + n % 977)
    table, ref = table_case('steps', n, supports, x, 3100 + n % 977, lift=range(len(steps)))
    lifted = np.sum(np.abs(table[:len(steps)]) ** 2, axis=1)
    last2 = np.array([np.sum(np.abs(table[i, k - 2:k]) ** 2) for i, k in enumerate(supports[:len(steps)])])
    assert np.all(np.abs(last2 / lifted - 0.25) < 1e-9)
    km = whole_and_chunked(n, dtype, F, attach_table(table), x, ref, f'table need steps n=2^{n.bit_length() - 1}',
                           monkeypatch)
    np.testing.assert_array_equal(km, np.array(supports) - 1)
    for (q, off), k in zip(steps, km[:len(steps)]):
        g = (off - 1) // 4                                              # the group the step falls into
        first, last = V.need(k, 4 * g, n1, t), V.need(k, 4 * g + 3, n1, t)
        assert (first, last) == (q + 1, q), (q, off, first, last)
        assert V.variant(first, lad) > V.variant(last, lad) == q


# ------------------------------------------------------------------ analytic rows
def pick_analytic(n, dtype, kind):
    """Nine of ~160 candidate frequencies: per variant of the ladder the candidate whose km lies
    deepest inside the variant's range of bins (need equal at the first and the last row), then
    the next deepest ones of any variant.  -> (freqs, their NZ)"""
    n1, n2, e, t, lad = geometry(n, dtype, False)
    bins = n // e
    cand = np.geomspace(0.6, 480., 160)
    km = support(n, dtype, kind, cand)
    depth = {}
    for f, k in zip(cand, km):
        a, b = row_variants(k, n1, t, lad)
        if a == b:
            lo = max([v for v in lad if v < a], default=0)
            depth[float(f)] = (a, min(k - lo * bins, a * bins - 1 - k))
    order = sorted(depth, key=lambda f: -depth[f][1])
    chosen = [next((f for f in order if depth[f][0] == nz), None) for nz in sorted(lad)]
    missing = [nz for nz, f in zip(sorted(lad), chosen) if f is None]
    assert not missing, f'no candidate frequency runs the variants {missing} ({kind}, n={n}, {dtype})'
    chosen += [f for f in order if f not in chosen][:9 - len(chosen)]
    assert len(chosen) == 9
    return sorted(chosen), lad


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', ROW_SIZES)
@pytest.mark.parametrize('kind', ['morse', 'morlet'])
def test_analytic_rows_every_variant(kind, n, dtype, monkeypatch):
    """Morse and Morlet rows steered into every NZ of their ladder (fp32 E = 32: steps of 4, from
    the LDS image up to NZ = 16 and from global memory above)."""
    n1, n2, e, t, _ = geometry(n, dtype, False)
    freqs, lad = pick_analytic(n, dtype, kind)
    x = noise(2, n, 4000 + n % 977)
    ref = cached('analytic', (kind, n, tuple(freqs)),
                 lambda: np.stack([O.cwt(kind, xi.astype(np.float64), freqs) for xi in x]))
    km = whole_and_chunked(n, dtype, len(freqs), attach_stock(kind, n, freqs), x, ref,
                           f'{kind} variants n=2^{n.bit_length() - 1}', monkeypatch)
    nz = [row_variants(k, n1, t, lad) for k in km]
    print(f'{kind} n=2^{n.bit_length() - 1} {dtype}: freqs {np.array2string(np.array(freqs), precision=4)} '
          f'NZ {[a for a, _ in nz]}')
    assert all(a == b for a, b in nz), nz
    hit = {a for a, _ in nz}
    assert hit == lad, f'row variants hit {sorted(hit)} != ladder {sorted(lad)}'
    if dtype == 'float32' and n2 >= 8192:
        src = {V.from_lds(e, dtype, False, a) for a in hit}
        assert src == {True, False}


def steer(n, kind, qs):
    """Per q a frequency whose fp32 support bound km (the plan's own row_support) has
    km // (n / 32) == q and km % (n / 32) in {0, 1, 2}.  km is linear in f to within a bin here
    (Morse: x = nu / f; Morlet: x = nu / f * sigma for f >= a few Hz), so one probe gives bins
    per Hz, then 301 candidates a quarter of a bin apart around each target go on one plan; a
    second round re-centres on the nearest candidate.  A target not reached fails."""
    bins = n // 32
    probe = np.arange(50., 401., 50.)
    slope = support(n, 'float32', kind, probe) / probe                    # bins per Hz
    found = {}
    centre = {q: (q * bins + 1) / slope[np.argmin(np.abs(probe * slope - q * bins))] for q in qs}
    for _ in range(2):
        todo = [q for q in qs if q not in found]
        if not todo:
            break
        cand = np.concatenate([centre[q] + np.arange(-150, 151) * 0.25 / slope[-1] for q in todo])
        km = support(n, 'float32', kind, cand)
        for i, q in enumerate(todo):
            f, k = cand[301 * i:301 * (i + 1)], km[301 * i:301 * (i + 1)]
            for want in (1, 0, 2):
                ok = np.nonzero((k // bins == q) & (k % bins == want))[0]
                if ok.size:
                    found[q] = float(f[ok[ok.size // 2]])
                    break
            else:
                j = np.argmin(np.abs(k - (q * bins + 1)))
                centre[q] = f[j] + (q * bins + 1 - k[j]) * (f[1] - f[0]) / 0.25
    missing = [q for q in qs if q not in found]
    assert not missing, f'no frequency with km = q n/32 + (0..2) for q in {missing} ({kind}, n={n})'
    return [found[q] for q in qs]


@pytest.mark.parametrize('n', [1 << 18, 1 << 19])
@pytest.mark.parametrize('kind', ['morse', 'morlet'])
def test_analytic_rows_across_the_dma_switch(kind, n, monkeypatch):
    """fp32 E = 32 rows whose need drops inside the first four-row workgroup: at q = 16 it runs
    NZ = 20 from global memory and then NZ = 16 from an Xt row DMA'd into LDS in the middle of its
    loop; at q = 4, 8 and 12 the DMA round count changes between consecutive rows; at q = 20 and
    24 the variant changes among the rows read from global memory."""
    dtype = 'float32'
    n1, n2, e, t, lad = geometry(n, dtype, False)
    assert e == 32 and lad == {4, 8, 12, 16, 20, 24, 32}
    bins = n // 32
    qs = [4, 8, 12, 16, 20, 24]
    steered = steer(n, kind, qs)
    freqs = steered + [3., 60., 250.]
    x = noise(2, n, 5000 + n % 977)
    ref = np.stack([O.cwt(kind, xi.astype(np.float64), freqs) for xi in x])
    km = whole_and_chunked(n, dtype, len(freqs), attach_stock(kind, n, freqs), x, ref,
                           f'{kind} DMA switch n=2^{n.bit_length() - 1}', monkeypatch)
    print(f'{kind} n=2^{n.bit_length() - 1}: steered f {[f"{f:.6f}" for f in steered]} km - q n/32 '
          f'{[int(k - q * bins) for q, k in zip(qs, km)]}')
    for q, k in zip(qs, km):
        assert k // bins == q and k % bins in (0, 1, 2), (q, k)
        first, last = V.need(k, 0, n1, t), V.need(k, 3, n1, t)
        assert (first, last) == (q + 1, q), (q, k, first, last)
        assert V.variant(last, lad) == q < V.variant(first, lad)
    k16 = km[qs.index(16)]
    assert not V.from_lds(e, dtype, False, V.variant(V.need(k16, 0, n1, t), lad))
    assert V.from_lds(e, dtype, False, V.variant(V.need(k16, 3, n1, t), lad))
