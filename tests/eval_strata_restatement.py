"""Shared by test_eval_strata_cpu.py and test_gpu_eval_strata.py: an independent NumPy restatement of the
stratified evaluation (include/cad/cad.h, "stratified evaluation").  Bin ids are computed in np.float32 with
exactly the operation order stated there; a stratum's expected sums are eval_restatement.ref_sums with the
stratum's pixels as the mask, so the twelve terms are restated only once."""
import numpy as np

import eval_restatement as R

DEPTH_CUTS = (1.0, 2.0, 3.0, 5.0)
ANGLE_CUTS = (10.0, 20.0, 30.0)
MARGIN = 1e-6   # relative distance every rho^2 keeps from every threshold (about 16 fp32 ulp)


def make_K(B, H, W):
    """(B,3,3) float32: an off-centre principal point and fx != fy, different per sample."""
    K = np.zeros((B, 3, 3), np.float32)
    for b in range(B):
        K[b] = [[0.9 * W * (1 + 0.07 * b), 0.0, W / 2 - 0.37 + 0.5 * b],
                [0.0, 0.92 * W * (1 + 0.07 * b), H / 2 + 0.21 - 0.3 * b],
                [0.0, 0.0, 1.0]]
    return K


def angle_thresholds(cuts_deg):
    """t_j = (float)(tan(theta_j pi / 180)^2), tangent and square in double, rounded once."""
    return np.float32(np.tan(np.deg2rad(np.asarray(cuts_deg, np.float64))) ** 2)


def depth_bins(gt, cuts):
    """(B,1,H,W) int: the number of cuts c_j <= gt, compared in fp32."""
    g = np.asarray(gt, np.float32)
    out = np.zeros(g.shape, np.int64)
    for c in np.asarray(cuts, np.float32):
        out += (c <= g)
    return out


def rho2(K, H, W):
    """(B,1,H,W) float32: x = (u - cx) / fx, y = (v - cy) / fy, rho2 = x x + y y, each operation rounded to
    fp32 (NumPy float32 arithmetic rounds every operation)."""
    K = np.asarray(K, np.float32).reshape(-1, 9)
    u = np.arange(W, dtype=np.float32)[None, None, None, :]
    v = np.arange(H, dtype=np.float32)[None, None, :, None]
    fx, cx, fy, cy = (K[:, i].reshape(-1, 1, 1, 1) for i in (0, 2, 4, 5))
    with np.errstate(all="ignore"):
        x = (u - cx) / fx
        y = (v - cy) / fy
        xx = x * x
        yy = y * y
        r = xx + yy
    assert r.dtype == np.float32
    return np.broadcast_to(r, (K.shape[0], 1, H, W))


def angle_bins(K, H, W, cuts_deg, check_margin=True):
    """(B,1,H,W) int: the number of thresholds t_j <= rho2 (a NaN rho2: bin 0).  With check_margin no
    rho2 may lie within MARGIN relative of a threshold, which makes the membership independent of a
    last-bit difference."""
    r = rho2(K, H, W)
    t = angle_thresholds(cuts_deg)
    if check_margin:
        rel = np.abs(r.astype(np.float64)[..., None] / t.astype(np.float64) - 1.0)
        assert rel.min() > MARGIN, rel.min()
    out = np.zeros(r.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for tj in t:
            out += (tj <= r)
    return out


def ref_strata_sums(pred, gt, mask, bins, nbins, lo=0.1, hi=10.0, clamp=True):
    """(B, nbins, 12) float64: R.ref_sums restricted to the pixels of each bin."""
    B = pred.shape[0]
    out = np.zeros((B, nbins, 12), np.float64)
    for k in range(nbins):
        m = (bins == k)
        if mask is not None:
            m = m & (mask != 0)
        out[:, k] = R.ref_sums(pred, gt, m.astype(np.uint8), lo, hi, clamp)
    return out


def strata_summary(sums):
    """Per bin: R.summary over the samples with a valid pixel in the bin (count = their number); pooled over
    all samples.  A bin without a sample: zeros."""
    sums = np.asarray(sums, np.float64)
    out = []
    for k in range(sums.shape[1]):
        rows = sums[:, k]
        present = rows[rows[:, 0] > 0]
        if len(present):
            s = R.summary(present)
        else:
            s = {stat: np.zeros(12) for stat in ("mean", "std", "median", "min", "max", "pooled")}
        s["pooled"] = R.finish(rows.sum(0))[0]
        s["count"] = len(present)
        out.append(s)
    return out
