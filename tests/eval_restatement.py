"""Shared by test_eval_cpu.py and test_gpu_eval.py: the seeded inputs of the evaluation tests and an
independent float64 NumPy restatement of DepthMetrics::compute's twelve sums (include/cad/cad.h,
"offline evaluation").  The validity test and the clamp are done in fp32, exactly as stated there;
everything after that is float64."""
import functools

import numpy as np

KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "mae", "log10", "delta_1.25", "delta_1.25^2", "delta_1.25^3",
        "num_valid_pixels", "mean_pred_depth", "mean_gt_depth")
RANGES = ((0.1, 10.0), (0.5, 8.0))
# the thresholds as the reference forms them: fp32 products of 1.25f
T1 = np.float32(1.25)
T2 = np.float32(T1 * T1)
T3 = np.float32(np.float32(T1 * T1) * T1)
REAL = (1, 2, 3, 4, 5, 6, 10, 11)   # the real-valued sums (the rest are counts)


def _valid(g, m, lo, hi):
    v = (g > np.float32(lo)) & (g < np.float32(hi))
    return v if m is None else v & (m != 0)


def ref_sums(pred, gt, mask=None, lo=0.1, hi=10.0, clamp=True):
    """(B, 12) float64: {n, |d|/g, d^2/g, d^2, (ln p - ln g)^2, |d|, |log10 p - log10 g|, #(r<1.25),
    #(r<1.25^2), #(r<1.25^3), p, g} sums over the valid pixels of each sample."""
    B = pred.shape[0]
    out = np.zeros((B, 12), np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            p32, g32 = pred[b].reshape(-1), gt[b].reshape(-1)
            v = _valid(g32, None if mask is None else mask[b].reshape(-1), lo, hi)
            p32, g32 = p32[v], g32[v]
            if clamp:
                p32 = np.minimum(np.maximum(p32, np.float32(lo)), np.float32(hi))
            p, g = p32.astype(np.float64), g32.astype(np.float64)
            d = p - g
            r = np.maximum(p / g, g / p)
            out[b] = [p.size, (np.abs(d) / g).sum(), (d * d / g).sum(), (d * d).sum(), ((np.log(p) - np.log(g)) ** 2).sum(),
                      np.abs(d).sum(), np.abs(np.log10(p) - np.log10(g)).sum(), (r < np.float64(T1)).sum(),
                      (r < np.float64(T2)).sum(), (r < np.float64(T3)).sum(), p.sum(), g.sum()]
    return out


def finish(sums):
    """(N, 12) sums -> (N, 12) float64 metrics in KEYS order; a row with n = 0 gives zeros."""
    sums = np.asarray(sums, np.float64).reshape(-1, 12)
    m = np.zeros_like(sums)
    for i, t in enumerate(sums):
        n = t[0]
        if n > 0:
            m[i] = [t[1] / n, t[2] / n, np.sqrt(t[3] / n), np.sqrt(t[4] / n), t[5] / n, t[6] / n, t[7] / n, t[8] / n, t[9] / n,
                    n, t[10] / n, t[11] / n]
    return m


def summary(sums):
    """mean / population std / median / min / max over samples and the pooled metrics, float64."""
    m = finish(sums)
    return {"mean": m.mean(0), "std": m.std(0), "median": np.median(m, 0), "min": m.min(0), "max": m.max(0),
            "pooled": finish(np.asarray(sums, np.float64).reshape(-1, 12).sum(0))[0]}


def _near_threshold(pred, gt):
    """Pixels whose max(p/g, g/p) lies within 1e-4 relative of a threshold under any tested setting."""
    bad = np.zeros(pred.shape, bool)
    g = gt.astype(np.float64)
    with np.errstate(all="ignore"):
        for lo, hi in RANGES:
            for clamp in (False, True):
                p = (np.clip(pred, np.float32(lo), np.float32(hi)) if clamp else pred).astype(np.float64)
                r = np.maximum(p / g, g / p)
                for t in (T1, T2, T3):
                    bad |= np.abs(r / np.float64(t) - 1.0) < 1e-4
    return bad & (gt > 0)


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, seed=0):
    """pred, gt (B,1,H,W) float32 and mask (B,1,H,W) uint8, seeded.  gt ~ U[0.05, 12] so both range bounds
    bite, ~5 % exactly 0, a few exactly on each tested min_depth / max_depth (invalid: the bounds are
    strict); pred = gt exp(U(-0.9, 0.9)) so every threshold has pixels on both sides, with a few <= 0 and
    a few above max_depth so the clamp matters; pixels within 1e-4 relative of a threshold are re-drawn,
    which makes the three counts and n exact.  Treat the arrays as read-only (cached)."""
    rng = np.random.default_rng(1000003 * seed + 10007 * B + 101 * H + W)
    n = B * H * W
    gt = rng.uniform(0.05, 12.0, n).astype(np.float32)
    gt[rng.random(n) < 0.05] = 0.0
    edge = rng.choice(n, size=min(n, 10), replace=False)
    for i, v in zip(edge, (0.1, 10.0, 0.5, 8.0, 0.1, 10.0, 0.5, 8.0, 0.0, 0.0)):   # (small shapes: zeros for certain)
        gt[i] = np.float32(v)
    pred = (gt * np.exp(rng.uniform(-0.9, 0.9, n))).astype(np.float32)
    free = np.setdiff1d(np.flatnonzero((gt > 0.6) & (gt < 7.9)), edge)
    odd = rng.choice(free, size=min(free.size, 6), replace=False)
    for i, v in zip(odd, (0.0, -1.5, 11.0, 25.0, -0.01, 10.5)):
        pred[i] = np.float32(v)
    fixed = np.zeros(n, bool)
    fixed[odd] = True
    for _ in range(100):
        bad = _near_threshold(pred, gt) & ~fixed
        if not bad.any():
            break
        k = int(bad.sum())
        pred[bad] = (gt[bad] * np.exp(rng.uniform(-0.9, 0.9, k))).astype(np.float32)
    assert not (_near_threshold(pred, gt)).any()
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    mask[mask != 0] = rng.integers(1, 256, int((mask != 0).sum()), dtype=np.uint8)   # nonzero, not just 1
    shp = (B, 1, H, W)
    return pred.reshape(shp), gt.reshape(shp), mask.reshape(shp)


def assert_sums_close(got, want, rtol=2e-5):
    """Counts exact; real-valued sums within rtol relative.  A sum the restatement finds non-finite (the
    log sums of unclamped predictions <= 0) must be non-finite in the same way."""
    got, want = np.asarray(got, np.float64).reshape(-1, 12), np.asarray(want, np.float64).reshape(-1, 12)
    assert got.shape == want.shape
    for k in (0, 7, 8, 9):
        assert np.array_equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    for k in REAL:
        for g, w in zip(got[:, k], want[:, k]):
            if np.isfinite(w):
                assert abs(g - w) <= rtol * abs(w), (k, g, w, abs(g - w) / max(abs(w), 1e-300))
            else:
                assert (np.isnan(w) and np.isnan(g)) or g == w, (k, g, w)
