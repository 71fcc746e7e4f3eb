"""NumPy model of the sampled white-balance tables (csrc/wb_predict.hip, csrc/wb_predict_device.h): the ranks of
np.percentile, the condition under which counts below and up to a predicted value prove a percentile exact, and the
confidence gate over 16 groups of sample histograms.  No GPU."""
import numpy as np

GROUPS = 16


def mark_ranks(n, k):
    """(lo, hi, t) of mark k (0: 2 %, 1: 98 %) among n samples, as numpy's 'linear' method and wb_mark_ranks compute them."""
    q = np.float64(2.0 if k == 0 else 98.0) / np.float64(100.0)
    vi = np.float64(n - 1) * q
    lo = int(np.floor(vi))
    return lo, min(lo + 1, n - 1), float(vi - np.float64(lo))


def mark_exact(hist, k, v):
    """wb_mark_exact: do lt = #(x < v) and le = #(x <= v) prove that the percentile of mark k is exactly v?  Both order statistics
    that carry weight must be v; with t == 0 the upper one carries none."""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist.sum())
    lt, le = int(hist[:v].sum()), int(hist[:v + 1].sum())
    lo, hi, t = mark_ranks(n, k)
    top = lo if t == 0.0 else hi
    return lt <= lo and le >= top + 1


def mark_value(hist, k):
    """(v, #(x < v), hist[v]): the value whose bin holds the lower order statistic of mark k."""
    hist = np.asarray(hist, dtype=np.int64)
    lo, _, _ = mark_ranks(int(hist.sum()), k)
    cum = np.cumsum(hist)
    v = int(np.searchsorted(cum, lo, side="right"))
    return v, int(cum[v] - hist[v]), int(hist[v])


def cdf_margin(hist, k):
    """(v, margin): how far, as a share of the samples, the mark lies from the nearer edge of the bin of v."""
    n = int(np.asarray(hist).sum())
    q = 0.02 if k == 0 else 0.98
    v, before, cnt = mark_value(hist, k)
    return v, min(q - before / n, (before + cnt) / n - q)


def predict(group_hists, kk=3):
    """k_wb_decide for one channel: group_hists [16][256] -> ((v_lo, v_hi), confident)."""
    g = np.asarray(group_hists, dtype=np.int64).reshape(GROUPS, 256)
    pooled = g.sum(axis=0)
    n = int(pooled.sum())
    values, confident = [], n > 0 and bool((g.sum(axis=1) > 0).all())
    for k in range(2):
        q = (2.0 if k == 0 else 98.0) / 100.0
        v, before, cnt = mark_value(pooled, k)
        values.append(v)
        for e in range(2):
            if (e == 0 and v == 0) or (e == 1 and v == 255) or not confident:
                continue
            f_g = g[:, :v + e].sum(axis=1) / g.sum(axis=1)
            se = max(np.sqrt(((f_g - f_g.mean()) ** 2).sum() / (GROUPS * (GROUPS - 1))), np.sqrt(q * (1.0 - q) / n))
            f = (before + (cnt if e else 0)) / n
            confident = confident and bool((f - q if e else q - f) >= kk * se)
    return tuple(values), confident
