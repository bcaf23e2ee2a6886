"""Shared by test_eval_align_cpu.py and test_gpu_eval_align.py: the inputs of the scale-alignment tests and
an independent sort-based / float64 NumPy restatement of the four alignment modes of include/cad/cad.h
("scale-aligned evaluation") and of the aligned sums.  The validity test, the median's midpoint, the
median ratio and the application of (scale, shift) are fp32, exactly as stated there; the statistics of
log_mean and scale_shift are float64, rounded to fp32 once."""
import functools

import numpy as np

import eval_restatement as R

MODES = ("none", "median", "log_mean", "scale_shift")
FACTORS = (0.011, 0.37, 2.9)   # per-sample factors on pred, far from 1: a kernel that forgets the scale cannot pass
F32 = np.float32


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, seed=0):
    """R.make_inputs with sample b's pred multiplied by FACTORS[b % 3] (fp32).  Read-only (cached)."""
    pred, gt, mask = R.make_inputs(B, H, W, seed)
    f = np.array([FACTORS[b % 3] for b in range(B)], F32).reshape(B, 1, 1, 1)
    return (pred * f).astype(F32), gt, mask


def valid(gt, mask, lo, hi):
    """Boolean valid set of one sample (flat)."""
    g = gt.reshape(-1)
    v = (g > F32(lo)) & (g < F32(hi))
    return v if mask is None else v & (mask.reshape(-1) != 0)


def median32(v):
    """(v_sorted[(n-1)/2] + v_sorted[n/2]) * 0.5f in fp32; 0 for an empty set."""
    if v.size == 0:
        return F32(0)
    s = np.sort(v.astype(F32))
    n = s.size
    return F32(F32(s[(n - 1) // 2] + s[n // 2]) * F32(0.5))


def ref_medians(pred, gt, mask=None, lo=0.1, hi=10.0):
    """(B, 2) float32 {med_pred, med_gt} over each sample's valid pixels."""
    out = np.zeros((pred.shape[0], 2), F32)
    for b in range(pred.shape[0]):
        v = valid(gt[b], None if mask is None else mask[b], lo, hi)
        out[b] = median32(pred[b].reshape(-1)[v]), median32(gt[b].reshape(-1)[v])
    return out


def ref_stats(pred, gt, mask=None, lo=0.1, hi=10.0):
    """(B, 7) float64 {n, n_pos, sum p, sum g, sum p^2, sum pg, sum(ln g - ln p) over p > 0}."""
    out = np.zeros((pred.shape[0], 7), np.float64)
    for b in range(pred.shape[0]):
        v = valid(gt[b], None if mask is None else mask[b], lo, hi)
        p, g = pred[b].reshape(-1)[v].astype(np.float64), gt[b].reshape(-1)[v].astype(np.float64)
        pos = p > 0
        out[b] = [p.size, pos.sum(), p.sum(), g.sum(), (p * p).sum(), (p * g).sum(), (np.log(g[pos]) - np.log(p[pos])).sum()]
    return out


def solve(mode, stats, med):
    """One sample: (scale, shift) float32 and whether the mode's own formula applied (False: a fallback)."""
    n, npos, sp, sg, spp, spg, sl = (float(x) for x in stats)
    one = (F32(1), F32(0))
    if mode == "none":
        return one + (True,)
    if n <= 0:
        return one + (False,)
    if mode == "median":
        if not med[0] > 0:
            return one + (False,)
        return F32(F32(med[1]) / F32(med[0])), F32(0), True
    if mode == "log_mean":
        if npos <= 0:
            return one + (False,)
        return F32(np.exp(sl / npos)), F32(0), True
    assert mode == "scale_shift"
    det = n * spp - sp * sp
    if det > 0:
        s = (n * spg - sp * sg) / det
        return F32(s), F32((sg - s * sp) / n), True
    if spp > 0:
        return F32(spg / spp), F32(0), False
    return one + (False,)


def ref_alignment(mode, pred, gt, mask=None, lo=0.1, hi=10.0):
    """(B, 2) float32 (scale, shift) and (B,) bool aligned flags."""
    st, med = ref_stats(pred, gt, mask, lo, hi), ref_medians(pred, gt, mask, lo, hi)
    rows = [solve(mode, st[b], med[b]) for b in range(pred.shape[0])]
    return np.array([[r[0], r[1]] for r in rows], F32).reshape(-1, 2), np.array([r[2] for r in rows], bool)


def apply(pred, st):
    """scale * pred + shift per sample: one fp32 multiply, one fp32 add."""
    st = np.asarray(st, F32).reshape(-1, 2)
    out = np.empty_like(pred)
    for b in range(pred.shape[0]):
        out[b] = (st[b, 0] * pred[b]).astype(F32) + st[b, 1]
    return out


def ref_aligned_sums(pred, gt, mask, lo, hi, clamp, st):
    """(B, 12) float64 sums of R.ref_sums on the aligned prediction."""
    return R.ref_sums(apply(pred, st), gt, mask, lo, hi, clamp)


def near_threshold_counts(pred, gt, mask, lo, hi, clamp, st, band=1e-5):
    """(B, 3) int: each sample's valid pixels whose restated ratio max(p/g, g/p) of the aligned (and clamped)
    prediction lies within `band` relative of 1.25, 1.25^2, 1.25^3."""
    ap = apply(pred, st)
    out = np.zeros((pred.shape[0], 3), np.int64)
    with np.errstate(all="ignore"):
        for b in range(pred.shape[0]):
            v = valid(gt[b], None if mask is None else mask[b], lo, hi)
            p, g = ap[b].reshape(-1)[v], gt[b].reshape(-1)[v].astype(np.float64)
            if clamp:
                p = np.minimum(np.maximum(p, F32(lo)), F32(hi))
            p = p.astype(np.float64)
            r = np.maximum(p / g, g / p)
            out[b] = [(np.abs(r / np.float64(t) - 1.0) < band).sum() for t in (R.T1, R.T2, R.T3)]
    return out


def assert_aligned_sums_close(got, want, near, rtol=2e-5):
    """n exact; each threshold count within the sample's near-threshold pixel count; real-valued sums
    within rtol relative (non-finite where the restatement is, in the same way)."""
    got, want = np.asarray(got, np.float64).reshape(-1, 12), np.asarray(want, np.float64).reshape(-1, 12)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), (got[:, 0], want[:, 0])
    for j, k in enumerate((7, 8, 9)):
        assert (np.abs(got[:, k] - want[:, k]) <= near[:, j]).all(), (k, got[:, k], want[:, k], near[:, j])
    for k in R.REAL:
        for g, w in zip(got[:, k], want[:, k]):
            if np.isfinite(w):
                assert abs(g - w) <= rtol * abs(w), (k, g, w, abs(g - w) / max(abs(w), 1e-300))
            else:
                assert (np.isnan(w) and np.isnan(g)) or g == w, (k, g, w)


def ulp_diff(a, b):
    """Distance of two float32 values in units in the last place (ordered-integer difference)."""
    def key(x):
        i = int(np.asarray(x, F32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))
