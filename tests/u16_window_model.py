"""A NumPy / float64 model of the value-window pre-pass of uint16 tiles (lars_image_processing_amd/csrc/u16.hip), line by line:
which pixels the subsample sees (k_u16_sample12), the windows it predicts (k_u16_window) and whether each of the four order
statistics np.percentile needs lies inside its window (k_u16_count_win + k_u16_pick_win).  The kernels' arithmetic is the
specification; nothing here is tuned to what a device returned."""
import math

import numpy as np

EVERY = 64               # lars_d_wb_prepare samples every 64th stretch
STRETCH_QUADS = 1024     # quads (4 pixels) per stretch: one per lane of a workgroup
SAMPLE_BINS = 4096       # U16_SAMPLE_BINS: v >> 4
SAMPLE_SPAN = 16         # U16_SAMPLE_SPAN
WIN_MAX = 1024           # U16_WIN_MAX
MARKS = (0.02, 0.98)


def takes_window_route(ntiles, npix):
    """lars_d_wb_prepare's `fast && cap >= 64` for 3-channel, 4-byte aligned uint16 tiles (u16_hist_impl other than 1)."""
    fast = (ntiles == 1 or npix % 4 == 0) and npix * 6 < (1 << 30)
    return fast and (npix // 4 + 1023) // 1024 >= 64


def launch_geometry(ntiles, npix, every=EVERY):
    """(gridDim.x of the pre-pass's data kernels, sampled stretches per tile): the two-in-flight branch of k_u16_sample12
    runs where the second exceeds the first."""
    want = (1024 + ntiles - 1) // ntiles
    cap = (npix // 4 + 1023) // 1024
    want = max(1, min(want, cap))
    nstretch = ((npix >> 2) + STRETCH_QUADS - 1) // STRETCH_QUADS
    return want, (nstretch + every - 1) // every


def sampled_pixels(npix, every=EVERY):
    """Indices of the pixels k_u16_sample12 counts: every `every`-th stretch of 1024 quads, quads below npix >> 2 only (the
    npix & 3 tail pixels are never sampled)."""
    nquads = npix >> 2
    nstretch = (nquads + STRETCH_QUADS - 1) // STRETCH_QUADS
    nsampled = (nstretch + every - 1) // every
    quads = (np.arange(nsampled, dtype=np.int64)[:, None] * (every * STRETCH_QUADS) + np.arange(STRETCH_QUADS, dtype=np.int64)[None, :]).ravel()
    quads = quads[quads < nquads]
    return (quads[:, None] * 4 + np.arange(4, dtype=np.int64)[None, :]).ravel()


def ranks(npix):
    """The four ranks np.percentile(x, (2, 98)) reads: floor((n - 1) q) and the next one, per mark; and the two weights."""
    out, tq = [], []
    for q in (2.0 / 100.0, 98.0 / 100.0):
        vi = float(npix - 1) * q
        fl = math.floor(vi)
        out += [int(fl), min(int(fl) + 1, npix - 1)]
        tq.append(vi - fl)
    return out, tq


def windows(channel, every=EVERY, test_wrong=False):
    """k_u16_window on the 12-bit histogram of the channel's sampled pixels: ((lo, wd) of the 2 % mark, (lo, wd) of the 98 % mark).
    `channel`: the tile's samples of one channel in pixel order.  test_wrong: u16_hist_impl = 3."""
    channel = np.asarray(channel).ravel()
    hist = np.bincount(channel[sampled_pixels(channel.size, every)].astype(np.int64) >> 4, minlength=SAMPLE_BINS)
    total = int(hist.sum())
    cum = np.cumsum(hist)
    first_last = [[SAMPLE_BINS, 0], [SAMPLE_BINS, 0]]                       # first = 4096, last = 0: no window
    if total > 0:
        for k, q in enumerate(MARKS):
            spread = 4.0 * math.sqrt(float(total) * q * (1.0 - q)) + 2.0
            centre = float(total - 1) * q
            rl, rh = math.floor(centre - spread), math.ceil(centre + spread + 1.0)
            rl = max(rl, 0.0)
            rh = min(rh, float(total - 1))
            for e, r in enumerate((int(rl), int(rh))):
                first_last[k][e] = int(np.searchsorted(cum, r, side="right"))   # the bin with cum_before <= r < cum_before + count
    lo, wd = [0, 0], [0, 0]
    for k in range(2):
        first = max(first_last[k][0] - 1, 0)
        last = min(first_last[k][1] + 1, SAMPLE_BINS - 1)
        nb = last - first + 1
        ok = first_last[k][0] < SAMPLE_BINS and nb >= 1 and nb * SAMPLE_SPAN <= WIN_MAX
        lo[k] = first * SAMPLE_SPAN if ok else 0
        wd[k] = nb * SAMPLE_SPAN if ok else 0
        if test_wrong:
            lo[k], wd[k] = 0, SAMPLE_SPAN
    widest = max(wd)
    wd = [widest if w else 0 for w in wd]                                   # both windows as wide as the wider one
    return (lo[0], wd[0]), (lo[1], wd[1])


def order_statistics(channel):
    """The values at ranks() of the channel."""
    s = np.sort(np.asarray(channel).ravel())
    r, _ = ranks(s.size)
    return [int(s[i]) for i in r]


def verdict(channel, every=EVERY, test_wrong=False):
    """For each of the four ranks whether its order statistic lies in [lo, lo + wd) of its mark's window: what k_u16_pick_win's
    s_found[] holds (the counting pass knows how many samples lie below the window and the histogram inside it)."""
    win = windows(channel, every, test_wrong)
    vals = order_statistics(channel)
    return tuple(bool(win[j >> 1][1] and win[j >> 1][0] <= vals[j] < win[j >> 1][0] + win[j >> 1][1]) for j in range(4))


def tile_windows(tile, every=EVERY, test_wrong=False):
    """uint32[3][4] as lars_u16_window_report lays a tile's windows out: lo[0], lo[1], wd[0], wd[1] per channel."""
    out = np.zeros((3, 4), np.uint32)
    for c in range(3):
        (l0, w0), (l1, w1) = windows(tile[..., c].ravel(), every, test_wrong)
        out[c] = (l0, l1, w0, w1)
    return out


def tile_verdicts(tile, every=EVERY, test_wrong=False):
    return tuple(verdict(tile[..., c].ravel(), every, test_wrong) for c in range(3))


def tile_flag(tile, every=EVERY, test_wrong=False):
    """1 if any of the tile's 12 verdicts is false: the tile takes the two radix passes."""
    return int(not all(all(v) for v in tile_verdicts(tile, every, test_wrong)))


def percentiles(channel):
    """numpy's 'linear' rule with _lerp on the verdict's own order statistics, in float64 as k_u16_pick_win computes it."""
    vals = order_statistics(channel)
    _, tq = ranks(np.asarray(channel).size)
    out = []
    for k in range(2):
        a, b, t = float(vals[2 * k]), float(vals[2 * k + 1]), tq[k]
        d = b - a
        r = a + d * t
        if t >= 0.5:
            r = b - d * (1.0 - t)
        out.append(r)
    return out
