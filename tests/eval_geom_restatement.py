"""Shared by test_eval_geom_cpu.py and test_gpu_eval_geom.py: the seeded inputs of the geometric-evaluation
tests and an independent NumPy restatement of include/cad/cad.h, "geometric evaluation": surface normals of
a depth map from K by central differences in the cancellation-free closed form, the angular error between
the prediction's and the ground truth's normals, and the 3-D point error.

The validity test, the alignment (scale * pred + shift) and the clamp are fp32, exactly as stated there;
everything after that is float64 (dtype=np.float64, the yardstick).  dtype=np.float32 runs the same
operations individually rounded to fp32; it is used only to measure how far fp32 arithmetic may stray from
the yardstick per pixel (test_eval_geom_cpu.py), which is where the GPU tolerance comes from.

Tolerances (derived, not tuned):
  TOL_PIXEL   per-pixel bound on |theta_device - theta_fp64| in degrees: 8 x the largest fp32-vs-fp64
              difference of this restatement on these very inputs (MEASURED_FP32_DEG, re-measured and asserted
              by test_eval_geom_cpu.py), the allowance for FMA contraction and another atan2f.
  THRESHOLD_GAP  the makers keep every fp64 theta at least 10 x TOL_PIXEL away from 11.25 / 22.5 / 30 under
              every configuration the GPU test runs, so the three counts are exact.
  sums        sum theta within n TOL_PIXEL; sum theta^2 within 2 TOL_PIXEL sum theta + n TOL_PIXEL^2 plus the
              fp32 rounding of theta * theta (2^-23 relative); sum e / sum e^2: e is eight fp32 operations from
              exact inputs (two subtractions, two divisions, two squares, two additions, sqrtf, a product: at
              most 10 roundings of 2^-24), so 1e-6 / 2e-6 relative.
"""
import functools

import numpy as np

import eval_align_restatement as A

F32 = np.float32
KEYS = ("normal_mean", "normal_median", "normal_rmse", "normal_11.25", "normal_22.5", "normal_30", "num_normal_pixels",
        "point_mae", "point_rmse")
THRESHOLDS = (11.25, 22.5, 30.0)
LO, HI = 0.1, 10.0
# (B, H, W) of the GPU tests: one interior pixel; no interior pixel (twice); small odd; no multiple of 4 / 16 / 64
# with the halo column on a strip boundary; two blocks; two 64-column strip boundaries
SHAPES = ((1, 3, 3), (1, 2, 9), (1, 9, 2), (1, 5, 7), (3, 50, 70), (2, 64, 96), (2, 16, 130))
# every shape a GPU test runs: SHAPES, the batch-split test's and the allocation test's
ALL_SHAPES = SHAPES + ((6, 50, 70), (2, 16, 16))
# largest |theta_fp32 - theta_fp64| of this restatement over every shape and configuration below, degrees
# (test_eval_geom_cpu.py::test_fp32_conditioning prints and re-asserts it)
MEASURED_FP32_DEG = 2.3e-5
TOL_PIXEL = 8 * MEASURED_FP32_DEG
THRESHOLD_GAP = 10 * TOL_PIXEL
# configurations of the GPU agreement test: (scaled inputs, masked, clamp_pred, alignment mode)
CONFIGS = ((False, False, False, "none"), (False, False, True, "none"), (False, True, False, "none"),
           (False, True, True, "none"), (True, True, True, "median"), (True, True, True, "log_mean"),
           (True, True, True, "scale_shift"))
DEG = 180.0 / np.pi


def make_K(B, H, W):
    """(B,3,3) float32: fx != fy, an off-centre, non-integer principal point, different per sample."""
    K = np.zeros((B, 3, 3), F32)
    for b in range(B):
        K[b] = [[1.1 * W * (1 + 0.05 * b), 0, 0.5 * W - 0.5 + 0.37 + 0.6 * b],
                [0, 1.17 * W * (1 - 0.03 * b), 0.5 * H - 0.5 - 0.21 + 0.45 * b],
                [0, 0, 1]]
    return K


def rays(K, H, W, dtype=np.float64):
    """x = (u - cx) / fx, y = (v - cy) / fy of every pixel, (H,W) each; u, v the fp32 pixel indices."""
    T = dtype
    fx, cx, fy, cy = T(K[0, 0]), T(K[0, 2]), T(K[1, 1]), T(K[1, 2])
    u = np.arange(W, dtype=F32).astype(T)[None, :].repeat(H, 0)
    v = np.arange(H, dtype=F32).astype(T)[:, None].repeat(W, 1)
    return ((u - cx) / fx).astype(T), ((v - cy) / fy).astype(T)


def closed_form(d, K, dtype=np.float64):
    """c of the closed form at the interior pixels of depth map d (H,W): (3, H-2, W-2), every operation rounded
    to `dtype`."""
    T = dtype
    H, W = d.shape
    d = d.astype(T)
    fx, fy = T(K[0, 0]), T(K[1, 1])
    x, y = rays(K, H, W, T)
    x, y = x[1:-1, 1:-1], y[1:-1, 1:-1]
    dl, dr, du, dd = d[1:-1, :-2], d[1:-1, 2:], d[:-2, 1:-1], d[2:, 1:-1]
    with np.errstate(all="ignore"):
        a = dr - dl
        Aa = (dr + dl) / fx
        b = dd - du
        Bb = (dd + du) / fy
        c0 = -(a * Bb)
        c1 = -(Aa * b)
        c2 = ((Aa * Bb) + ((x * a) * Bb)) + ((y * Aa) * b)
    return np.stack([c0, c1, c2]).astype(T)


def differenced(d, K):
    """The same vector by differencing the back-projected points P = (x d, y d, d) in float64:
    (P(u+1,v) - P(u-1,v)) x (P(u,v+1) - P(u,v-1)), which equals c."""
    H, W = d.shape
    x, y = rays(K, H, W)
    d = d.astype(np.float64)
    P = np.stack([x * d, y * d, d])
    du = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    dv = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    return np.cross(du, dv, axis=0)


def unit(c, dtype=np.float64):
    """n = -c / |c| and whether c is finite with |c| > 0."""
    T = dtype
    with np.errstate(all="ignore"):
        ln = np.sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]).astype(T)).astype(T)
        ok = np.isfinite(ln) & (ln > 0)
        n = (-c / np.where(ok, ln, T(1))).astype(T)
    return n, ok


def angle(npred, ngt, dtype=np.float64):
    """atan2(|n_p x n_g|, n_p . n_g) in degrees."""
    T = dtype
    p, g = npred, ngt
    x0 = (p[1] * g[2] - p[2] * g[1]).astype(T)
    x1 = (p[2] * g[0] - p[0] * g[2]).astype(T)
    x2 = (p[0] * g[1] - p[1] * g[0]).astype(T)
    s = np.sqrt(((x0 * x0 + x1 * x1) + x2 * x2).astype(T)).astype(T)
    c = ((p[0] * g[0] + p[1] * g[1]) + p[2] * g[2]).astype(T)
    return (np.arctan2(s, c).astype(T) * T(F32(DEG) if T is F32 else DEG)).astype(T)


def valid_set(gt, mask, lo=LO, hi=HI):
    v = (gt > F32(lo)) & (gt < F32(hi))
    return v if mask is None else v & (mask != 0)


def five(valid):
    """(H,W) bool: the pixel is interior and it and its four neighbours are in `valid`."""
    out = np.zeros(valid.shape, bool)
    if valid.shape[0] >= 3 and valid.shape[1] >= 3:
        out[1:-1, 1:-1] = valid[1:-1, 1:-1] & valid[1:-1, :-2] & valid[1:-1, 2:] & valid[:-2, 1:-1] & valid[2:, 1:-1]
    return out


def scored(pred, gt, mask, lo, hi, clamp, st=None):
    """The prediction the metrics pass scores: clamp(scale * pred + shift), fp32."""
    p = pred if st is None else A.apply(pred, st)
    if clamp:
        with np.errstate(all="ignore"):
            p = np.minimum(np.maximum(p, F32(lo)), F32(hi))
    return p.astype(F32)


def theta_map(p, g, valid, K, dtype=np.float64):
    """One sample: (theta (H,W) in degrees, 0 where not normal-valid; normal-valid (H,W) bool).  p: the scored
    prediction, g: gt, both (H,W) fp32."""
    H, W = g.shape
    th = np.zeros((H, W), dtype)
    nv = five(valid)
    if not nv.any():
        return th, nv
    npd, okp = unit(closed_form(p, K, dtype), dtype)
    ngt, okg = unit(closed_form(g, K, dtype), dtype)
    nv[1:-1, 1:-1] &= okp & okg
    with np.errstate(all="ignore"):
        t = angle(npd, ngt, dtype)
    th[1:-1, 1:-1] = np.where(nv[1:-1, 1:-1], t, 0)
    return th, nv


def median32(theta, nv):
    """(sorted[(n-1)/2] + sorted[n/2]) * 0.5 of theta over nv; 0 for an empty set."""
    v = np.sort(theta[nv].reshape(-1))
    n = v.size
    return 0.0 if n == 0 else float((v[(n - 1) // 2] + v[n // 2]) * 0.5)


def ref_geom(pred, gt, mask, K, lo=LO, hi=HI, clamp=True, st=None, dtype=np.float64):
    """-> sums (B,8) float64 {n_normal, theta, theta^2, #<11.25, #<22.5, #<30, e, e^2}, medians (B,), theta maps
    (B,H,W), normal-valid maps (B,H,W), valid counts (B,)."""
    B, _, H, W = gt.shape
    p = scored(pred, gt, mask, lo, hi, clamp, st)
    sums, med = np.zeros((B, 8)), np.zeros(B)
    ths, nvs, ns = np.zeros((B, H, W), dtype), np.zeros((B, H, W), bool), np.zeros(B)
    for b in range(B):
        v = valid_set(gt[b, 0], None if mask is None else mask[b, 0], lo, hi)
        th, nv = theta_map(p[b, 0], gt[b, 0], v, K[b], dtype)
        x, y = rays(K[b], H, W, dtype)
        with np.errstate(all="ignore"):
            e = (np.abs(p[b, 0].astype(dtype) - gt[b, 0].astype(dtype)) * np.sqrt((1 + x * x) + y * y))[v].astype(np.float64)
        t = th[nv].astype(np.float64)
        sums[b] = [t.size, t.sum(), (t * t).sum()] + [(t < c).sum() for c in THRESHOLDS] + [e.sum(), (e * e).sum()]
        med[b] = median32(th, nv)
        ths[b], nvs[b], ns[b] = th, nv, v.sum()
    return sums, med, ths, nvs, ns


def ref_normals(depth, K, mask=None, lo=LO, hi=HI):
    """cad.depth_normals restated in float64: normals (B,3,H,W), zeros where invalid, and valid (B,1,H,W) bool."""
    B, _, H, W = depth.shape
    n, ok = np.zeros((B, 3, H, W)), np.zeros((B, 1, H, W), bool)
    for b in range(B):
        d = depth[b, 0]
        with np.errstate(all="ignore"):
            v = np.isfinite(d) & (d > F32(lo)) & (d < F32(hi))
        if mask is not None:
            v &= mask[b, 0] != 0
        nv = five(v)
        if nv.any():
            nn, good = unit(closed_form(np.where(np.isfinite(d), d, 0), K[b]))
            nv[1:-1, 1:-1] &= good
            n[b][:, 1:-1, 1:-1] = np.where(nv[1:-1, 1:-1], nn, 0)
        ok[b, 0] = nv
    return n + 0.0, ok


def normal_rgb(n):
    """rint(255 * ((n_x + 1) / 2, (1 - n_y) / 2, (1 - n_z) / 2)) of normals (...,3) -> uint8, half to even."""
    n = np.asarray(n, np.float64)
    t = np.stack([(n[..., 0] + 1) / 2, (1 - n[..., 1]) / 2, (1 - n[..., 2]) / 2], -1)
    return np.rint(np.clip(t, 0, 1) * 255).astype(np.uint8)


def plane_depth(nrm, c, K, H, W):
    """Depth map (H,W) float64 of the plane nrm . X = c seen through K: d = c / (nrm . (x, y, 1))."""
    x, y = rays(K, H, W)
    return c / (nrm[0] * x + nrm[1] * y + nrm[2])


# ---------------- finish ----------------
def finish(sums, med, n_valid):
    """(N,8) sums, (N,) medians, (N,) valid counts -> (N,9) float64 metrics in KEYS order."""
    sums = np.asarray(sums, np.float64).reshape(-1, 8)
    m = np.zeros((sums.shape[0], 9))
    for i, t in enumerate(sums):
        if t[0] > 0:
            m[i, :7] = [t[1] / t[0], med[i], np.sqrt(t[2] / t[0]), t[3] / t[0], t[4] / t[0], t[5] / t[0], t[0]]
        if n_valid[i] > 0:
            m[i, 7:] = [t[6] / n_valid[i], np.sqrt(t[7] / n_valid[i])]
    return m


def summary(sums, med, n_valid):
    """The strata's rule: columns 0..6 over the samples with n_normal > 0, columns 7, 8 over those with a valid
    pixel; pooled adds all sums (its median is NaN); an empty set gives zeros."""
    sums = np.asarray(sums, np.float64).reshape(-1, 8)
    n_valid = np.asarray(n_valid, np.float64).reshape(-1)
    m = finish(sums, med, n_valid)
    out = {k: np.zeros(9) for k in ("mean", "std", "median", "min", "max")}
    sets = [sums[:, 0] > 0] * 7 + [n_valid > 0] * 2
    for k, sel in enumerate(sets):
        col = m[sel, k]
        if col.size:
            for name, f in (("mean", np.mean), ("std", np.std), ("median", np.median), ("min", np.min), ("max", np.max)):
                out[name][k] = f(col)
    out["count"] = sums.shape[0]
    out["count_normal"] = int((sums[:, 0] > 0).sum())
    out["count_point"] = int((n_valid > 0).sum())
    pooled = finish(sums.sum(0, keepdims=True), [0.0], [n_valid.sum()])[0] if sums.shape[0] else np.zeros(9)
    pooled[1] = np.nan
    out["pooled"] = pooled
    return out


# ---------------- inputs ----------------
def _surface(B, H, W, K, rng):
    """Smooth gt (a tilted plane plus sinusoids in the ray coordinates) and pred = gt + a smaller smooth
    perturbation, float32 (B,1,H,W)."""
    gt, pred = np.zeros((B, 1, H, W)), np.zeros((B, 1, H, W))
    for b in range(B):
        x, y = rays(K[b], H, W)
        ph = rng.uniform(0, 2 * np.pi, 6)
        z = 3.0 + 0.4 * b + 1.5 * x - 1.1 * y + 0.25 * np.sin(5 * x + ph[0]) + 0.2 * np.cos(4 * y + ph[1]) \
            + 0.15 * np.sin(3 * x - 4 * y + ph[2])
        amp = 0.12 + 0.1 * b
        pz = z + amp * np.sin(7 * x + ph[3]) * np.cos(6 * y + ph[4]) + 0.05 * np.cos(9 * (x + y) + ph[5]) + 0.03
        gt[b, 0], pred[b, 0] = z, pz
    return pred.astype(F32), gt.astype(F32)


def near_threshold(pred, gt, mask, K, configs, factors):
    """(B,H,W) bool: normal-valid pixels whose fp64 theta lies within THRESHOLD_GAP of a threshold under one of
    `configs` (entries of CONFIGS), and the nearest such distance met."""
    B, _, H, W = gt.shape
    bad, nearest = np.zeros((B, H, W), bool), np.inf
    for scaled, masked, clamp, mode in configs:
        p = (pred * factors).astype(F32) if scaled else pred
        m = mask if masked else None
        st = None if mode == "none" else A.ref_alignment(mode, p, gt, m, LO, HI)[0]
        _, _, th, nv, _ = ref_geom(p, gt, m, K, LO, HI, clamp, st)
        for c in THRESHOLDS:
            bad |= nv & (np.abs(th - c) < THRESHOLD_GAP)
            if nv.any():
                nearest = min(nearest, float(np.abs(th[nv] - c).min()))
    return bad, nearest


@functools.lru_cache(maxsize=None)
def make_inputs(B, H, W, seed=0):
    """-> pred, scaled pred, gt (B,1,H,W) float32, mask (B,1,H,W) uint8, K (B,3,3) float32, seeded and cached
    (read-only).  gt is smooth with ~1.5 % of the pixels pushed out of (0.1, 10) (0, 11, and the bounds
    themselves, which are invalid: strict); the mask has ~3 % single-pixel holes and one block hole; images
    under 200 pixels keep every pixel (their few interior pixels are the point).  scaled pred = pred x
    A.FACTORS[b % 3], for the alignment modes.  A pixel whose theta comes within THRESHOLD_GAP of a threshold
    under any of CONFIGS has its gt set to 0 (it leaves every valid set); that must cost at most 1 % of the
    normal-valid pixels (in practice nudging the prediction beside it suffices and none is removed)."""
    rng = np.random.default_rng(7919 * seed + 10007 * B + 101 * H + W)
    K = make_K(B, H, W)
    pred, gt = _surface(B, H, W, K, rng)
    mask = np.full((B, 1, H, W), 1, np.uint8)
    if H * W >= 200:
        n = B * H * W
        out = rng.choice(n, size=max(4, int(0.015 * n)), replace=False)
        gt.reshape(-1)[out] = np.resize(np.array([0.0, 11.0, 10.0, 0.1], F32), out.size)
        holes = rng.random((B, 1, H, W)) < 0.03
        mask[holes] = 0
        mask[:, :, H // 3:H // 3 + 4, W // 2:W // 2 + 5] = 0
        mask[mask != 0] = rng.integers(1, 256, int((mask != 0).sum()), dtype=np.uint8)   # nonzero, not just 1
        far = (slice(0, 1), slice(0, 1), slice(H - 8, H - 2), slice(2, 10))
        pred[far] += F32(8.0)   # above max_depth: the clamp matters
    factors = np.array([A.FACTORS[b % 3] for b in range(B)], F32).reshape(B, 1, 1, 1)
    before = gt.copy()
    for it in range(20):
        bad, _ = near_threshold(pred, gt, mask, K, CONFIGS, factors)
        if not bad.any():
            break
        # theta at (v, u) reads the four neighbours: nudge the prediction of the right-hand one by a fraction of
        # a millimetre (a few tenths of a degree); after a few rounds of that, drop the pixel from gt
        if it < 12:
            pred[:, 0, :, 1:][bad[:, :, :-1]] += F32(2e-4 * (1 + it))
        else:
            gt[:, 0][bad] = 0.0
    bad, nearest = near_threshold(pred, gt, mask, K, CONFIGS, factors)
    assert not bad.any(), "a theta stays within THRESHOLD_GAP of a threshold"
    lost = _lost_share(before, gt, mask)
    assert lost <= 0.01, f"conditioning removed {lost:.3%} of the normal-valid pixels"
    CONDITIONING[(B, H, W, seed)] = (lost, nearest)
    return pred, (pred * factors).astype(F32), gt, mask, K


CONDITIONING = {}   # (B, H, W, seed) -> (share of normal-valid pixels removed, nearest |theta - threshold|)


def _lost_share(before, after, mask):
    """Share of the five-pixel-valid pixels the conditioning cost: the worst sample, masked or not."""
    worst = 0.0
    for m in (None, mask):
        for b in range(before.shape[0]):
            mb = None if m is None else m[b, 0]
            n0, n1 = five(valid_set(before[b, 0], mb)).sum(), five(valid_set(after[b, 0], mb)).sum()
            if n0:
                worst = max(worst, (n0 - n1) / n0)
    return worst


# ---------------- comparisons ----------------
def assert_geom_close(got_sums, got_med, want_sums, want_med):
    """Counts exact; sum theta, sum theta^2 within the bounds derived from TOL_PIXEL; the point sums within
    1e-6 / 2e-6 relative; the median within TOL_PIXEL (module docstring)."""
    got, want = np.asarray(got_sums, np.float64).reshape(-1, 8), np.asarray(want_sums, np.float64).reshape(-1, 8)
    assert got.shape == want.shape
    for k in (0, 3, 4, 5):
        assert np.array_equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    n, s1, s2 = want[:, 0], want[:, 1], want[:, 2]
    d1, d2 = np.abs(got[:, 1] - s1), np.abs(got[:, 2] - s2)
    print("sum theta: |diff| / n", d1 / np.maximum(n, 1), " bound", TOL_PIXEL)
    assert (d1 <= n * TOL_PIXEL + 1e-12 * s1).all(), (got[:, 1], s1)
    assert (d2 <= 2 * TOL_PIXEL * s1 + n * TOL_PIXEL ** 2 + 2.0 ** -23 * s2).all(), (got[:, 2], s2)
    for k, r in ((6, 1e-6), (7, 2e-6)):
        assert (np.abs(got[:, k] - want[:, k]) <= r * np.abs(want[:, k])).all(), (k, got[:, k], want[:, k])
    dm = np.abs(np.asarray(got_med, np.float64) - np.asarray(want_med, np.float64))
    print("median: |diff|", dm)
    assert (dm <= TOL_PIXEL).all(), (got_med, want_med)
