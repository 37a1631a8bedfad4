"""What test_pac_bins_cpu.py and test_gpu_pac_bins.py share: the bin rule of nw_execute_pac_bins restated in numpy
(bin_of), the atan2 binning it stands for (atan2_bin) and the binned sums of rows in the contract's order
(binned_sums)."""
import numpy as np

from epoch_cases import lane_sum

from ninwavelets_amd import _lib as L


def bin_of(re, im, nbins):
    """THE BIN of ninwave.h for float64 arrays (re, im), on the library's own table: upper = im > 0 or
    (im == 0 and re > 0), base = h or 0, bin = base + the number of k = 1 .. h - 1 with c[base + k] im -
    s[base + k] re >= 0 (numpy rounds each product on its own), and h where re == im == 0."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    cs = L.pac_bin_edges(nbins)
    h = nbins // 2
    base = np.where((im > 0) | ((im == 0) & (re > 0)), h, 0)
    b = base.copy()
    with np.errstate(invalid='ignore'):
        for k in range(1, h):
            b += (cs[base + k, 0] * im - cs[base + k, 1] * re) >= 0
    return np.where((re == 0) & (im == 0), h, b)


def atan2_bin(re, im, nbins):
    """floor((atan2(im, re) + pi) / (2 pi / nbins)), the angle pi in bin 0."""
    return np.floor((np.arctan2(im, re) + np.pi) / (2 * np.pi / nbins)).astype(np.int64) % nbins


def binned_sums(rows, ip, ia, fph, fam, idx, nbins, ordered):
    """(S (E, P, Fp, Fa, nbins), count (E, C, Fp, nbins), bins (E, C, Fp, T), A (E, C, Fa, T)) of complex rows
    (E, C, F, n) over the samples ``idx``: bins by bin_of, A = hypot(re, im); ``ordered``: every sum in the
    contract's order (lane_sum of where(bin == b, A, 0.0)), otherwise numpy's."""
    yw = rows[..., idx]
    re, im = np.ascontiguousarray(yw.real, dtype=np.float64), np.ascontiguousarray(yw.imag, dtype=np.float64)
    A = np.hypot(re[:, :, fam], im[:, :, fam])                                     # (E, C, Fa, T)
    bins = bin_of(re[:, :, fph], im[:, :, fph], nbins)                             # (E, C, Fp, T)
    E, C = rows.shape[:2]
    S = np.empty((E, len(ip), len(fph), len(fam), nbins))
    count = np.empty((E, C, len(fph), nbins))
    Aa = A[:, ia][:, :, None]                                                      # (E, P, 1, Fa, T)
    for b in range(nbins):
        inb = bins == b
        count[..., b] = inb.sum(-1)
        terms = np.where(inb[:, ip][:, :, :, None], Aa, 0.0)                       # (E, P, Fp, Fa, T)
        S[..., b] = lane_sum(terms) if ordered else terms.sum(-1)
    return S, count, bins, A
