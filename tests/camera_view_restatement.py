"""NumPy restatement of the virtual-camera warp (include/cad/cad.h, "virtual cameras"; csrc/kernels/view_kernels.hip).

Conventions: pixel centres at integer coordinates, depth is Z along the optical axis, x right, y down, z forward,
skew ignored.  A view (zoom_x, zoom_y, shift_x, shift_y, yaw, pitch, roll) turns a sample's K into K' and rotates
the camera by R (P' = R P):

    fx' = zoom_x fx, fy' = zoom_y fy, cx' = cx + shift_x W, cy' = cy + shift_y H          (fp32 products and sums)
    R = Rz(roll) Rx(pitch) Ry(yaw),  Ry(t) = [[c,0,-s],[0,1,0],[s,0,c]],  Rx(t) = [[1,0,0],[0,c,-s],[0,s,c]],
    Rz(t) = [[c,-s,0],[s,c,0],[0,0,1]]                                       (double, rounded to fp32 once)

Per output pixel (u', v'): d' = ((u' - cx') / fx', (v' - cy') / fy', 1), d = R^T d', u = (fx d.x) / d.z + cx,
v = (fy d.y) / d.z + cy.  rgb: bilinear between floor and floor + 1 of the coordinate clamped to the image (edge
replicate), 0 where d.z <= 0 or the coordinate is not finite.  depth: nearest (floor(u + 0.5), floor(v + 0.5)),
Z' = Z / d.z where the tap is inside the image, d.z > 0, Z is finite and positive and the mask is non-zero; else 0.
An identity sample (R == I, K' == K bit for bit) is a copy.

warp() computes the coordinates twice: in float64 (the reference) and in float32 with every operation rounded in the
kernel's order (coords(..., np.float32)), which is what the device computes.  Nearest sampling is discontinuous, so
the two can pick different source pixels where u + 0.5 or v + 0.5 lies within delta of an integer (this includes the
inside / outside border) or d.z within delta of 0: `safe` leaves those pixels out of the depth and valid comparison.
Bilinear rgb is continuous and is compared everywhere."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
NEUTRAL = dict(zoom_x=1.0, zoom_y=1.0, shift_x=0.0, shift_y=0.0, yaw=0.0, pitch=0.0, roll=0.0)


def make_view(zoom=None, **kw):
    v = dict(NEUTRAL)
    if zoom is not None:
        v["zoom_x"] = v["zoom_y"] = zoom
    v.update(kw)
    return v


def make_K(B, H, W):
    """(B,3,3) float32 scaled to the shape: fx != fy, an off-centre, non-integer principal point, different per sample."""
    K = np.zeros((B, 3, 3), F32)
    for b in range(B):
        K[b] = [[0.9 * max(W, 4) * (1 + 0.07 * b), 0.0, W / 2 - 0.37 + 0.5 * b],
                [0.0, 0.92 * max(W, 4) * (1 + 0.07 * b), H / 2 + 0.21 - 0.3 * b],
                [0.0, 0.0, 1.0]]
    return K


def rotation(view):
    """R (3,3) float32 = Rz(roll) Rx(pitch) Ry(yaw): products in double, sums left to right, rounded to fp32 once."""
    rad = math.pi / 180.0
    cy, sy = math.cos(float(F32(view["yaw"])) * rad), math.sin(float(F32(view["yaw"])) * rad)
    cp, sp = math.cos(float(F32(view["pitch"])) * rad), math.sin(float(F32(view["pitch"])) * rad)
    cr, sr = math.cos(float(F32(view["roll"])) * rad), math.sin(float(F32(view["roll"])) * rad)
    Ry = [cy, 0.0, -sy, 0.0, 1.0, 0.0, sy, 0.0, cy]
    Rx = [1.0, 0.0, 0.0, 0.0, cp, -sp, 0.0, sp, cp]
    Rz = [cr, -sr, 0.0, sr, cr, 0.0, 0.0, 0.0, 1.0]

    def mul(a, b):
        return [(a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j] for i in range(3) for j in range(3)]
    return np.array([x + 0.0 for x in mul(Rz, mul(Rx, Ry))], F64).astype(F32).reshape(3, 3)


def resolve(view, K, H, W):
    """-> (K' (B,3,3) float32, R (B,3,3) float32) of one view against a batch's K."""
    K = np.asarray(K, F32)
    Kn = K.copy()
    Kn[:, 0, 0] = F32(view["zoom_x"]) * K[:, 0, 0]
    Kn[:, 1, 1] = F32(view["zoom_y"]) * K[:, 1, 1]
    Kn[:, 0, 2] = K[:, 0, 2] + F32(view["shift_x"]) * F32(W)
    Kn[:, 1, 2] = K[:, 1, 2] + F32(view["shift_y"]) * F32(H)
    return Kn, np.repeat(rotation(view)[None], K.shape[0], axis=0)


def coords(K, Kn, R, H, W, T=F64):
    """Source coordinate (u, v) and d.z of every output pixel of one sample, (H,W) each, every operation rounded to T
    in the kernel's order."""
    fx, cx, fy, cy = (T(K[0, 0]), T(K[0, 2]), T(K[1, 1]), T(K[1, 2]))
    fxn, cxn, fyn, cyn = (T(Kn[0, 0]), T(Kn[0, 2]), T(Kn[1, 1]), T(Kn[1, 2]))
    r = np.asarray(R, F32).astype(T).reshape(9)
    uo = np.arange(W, dtype=F32).astype(T)[None, :].repeat(H, 0)
    vo = np.arange(H, dtype=F32).astype(T)[:, None].repeat(W, 1)
    with np.errstate(all="ignore"):
        dx = (uo - cxn) / fxn
        dy = (vo - cyn) / fyn
        ex = (r[0] * dx + r[3] * dy) + r[6]
        ey = (r[1] * dx + r[4] * dy) + r[7]
        ez = (r[2] * dx + r[5] * dy) + r[8]
        u = (fx * ex) / ez + cx
        v = (fy * ey) / ez + cy
    assert u.dtype == T and v.dtype == T and ez.dtype == T
    return u, v, ez


def is_identity(K, Kn, R):
    same = all(F32(K[i, j]).tobytes() == F32(Kn[i, j]).tobytes() for i, j in ((0, 0), (0, 2), (1, 1), (1, 2)))
    return same and bool(np.all(np.asarray(R, F32) == np.eye(3, dtype=F32)))


def source_valid(depth, mask=None):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(depth) & (depth > 0)
    return ok if mask is None else ok & (mask != 0)


def warp_one(rgb, depth, mask, K, Kn, R, delta):
    """One sample: rgb (3,H,W), depth (H,W) float32, mask (H,W) or None -> dict (see warp)."""
    H, W = depth.shape
    ok_src = source_valid(depth, mask)
    if is_identity(K, Kn, R):
        z = np.zeros((H, W))
        return {"rgb": rgb.astype(F64), "depth": depth.copy(), "depth64": np.where(ok_src, depth, 0).astype(F64), "valid": ok_src,
                "safe": np.ones((H, W), bool), "u": z, "v": z, "dz": z + 1, "deviation": 0.0, "identity": True}
    u, v, dz = coords(K, Kn, R, H, W, F64)
    u32, v32, dz32 = coords(K, Kn, R, H, W, F32)
    with np.errstate(invalid="ignore"):
        front = dz > 0
        finite = np.isfinite(u) & np.isfinite(v)
    seen = front & finite
    us, vs = np.where(seen, u, 0.0), np.where(seen, v, 0.0)
    # bilinear rgb, edge replicate
    uc, vc = np.clip(us, 0, W - 1), np.clip(vs, 0, H - 1)
    x0, y0 = np.floor(uc).astype(np.int64), np.floor(vc).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    lx, ly = uc - x0, vc - y0
    src = rgb.astype(F64)
    out = np.zeros((3, H, W))
    for c in range(3):
        t0 = src[c, y0, x0] * (1 - lx) + src[c, y0, x1] * lx
        t1 = src[c, y1, x0] * (1 - lx) + src[c, y1, x1] * lx
        out[c] = np.where(seen, t0 * (1 - ly) + t1 * ly, 0.0)
    # nearest depth
    iu, iv = np.floor(us + 0.5), np.floor(vs + 0.5)
    inside = seen & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
    iu, iv = np.where(inside, iu, 0).astype(np.int64), np.where(inside, iv, 0).astype(np.int64)
    valid = inside & ok_src[iv, iu]
    zs = np.where(valid, depth[iv, iu], F32(1))
    with np.errstate(all="ignore"):
        d32 = np.where(valid, zs.astype(F32) / np.where(valid, dz32, F32(1)), F32(0)).astype(F32)   # the device's division
        d64 = np.where(valid, zs.astype(F64) / np.where(valid, dz, 1.0), 0.0)
    # pixels where fp32 and fp64 may pick different taps or sides
    with np.errstate(invalid="ignore"):
        fu, fv = us + 0.5, vs + 0.5
        near = (np.abs(fu - np.round(fu)) <= delta) | (np.abs(fv - np.round(fv)) <= delta)
        safe = np.isfinite(dz) & (np.abs(dz) > delta) & (~front | (finite & ~near))
        # the coordinate deviation where it matters: the pixels that look at (or next to) the image
        look = seen & (u > -1) & (u < W) & (v > -1) & (v < H)
        dev = float(max(np.abs(u32.astype(F64) - u)[look].max(initial=0.0), np.abs(v32.astype(F64) - v)[look].max(initial=0.0)))
    return {"rgb": out, "depth": d32, "depth64": d64, "valid": valid, "safe": safe, "u": u, "v": v, "dz": dz, "deviation": dev,
            "identity": False}


def warp(rgb, depth, mask, K, Kn, R, delta):
    """rgb (B,3,H,W), depth (B,1,H,W) float32, mask (B,1,H,W) or None, K, K', R (B,3,3) -> {"rgb" (B,3,H,W) float64,
    "depth" (B,1,H,W) float32 (the fp64 tap over the fp32 d.z, as the device divides), "depth64", "valid" (B,1,H,W) bool,
    "safe" (B,1,H,W) bool, "u", "v", "dz" (B,H,W) float64, "deviation": max |fp32 - fp64| coordinate over the pixels
    that look at the image, "identity": [bool per sample]}."""
    B = rgb.shape[0]
    per = [warp_one(rgb[b], depth[b, 0], None if mask is None else mask[b, 0], K[b], Kn[b], R[b], delta) for b in range(B)]
    out = {k: np.stack([p[k] for p in per]) for k in ("rgb", "u", "v", "dz")}
    for k in ("depth", "depth64", "valid", "safe"):
        out[k] = np.stack([p[k] for p in per])[:, None]
    out["deviation"] = max(p["deviation"] for p in per)
    out["identity"] = [p["identity"] for p in per]
    return out


def synth(B, H, W, seed=0, bad=True):
    """rgb U[0,1), a smooth depth field with holes (and, with bad, NaN, Inf and negative pixels), a mask that drops
    about 10 % of the pixels, K scaled to the shape."""
    rng = np.random.default_rng(1234 + seed + 17 * B + 131 * H + 977 * W)
    rgb = rng.random((B, 3, H, W), dtype=F32)
    vv, uu = np.mgrid[0:H, 0:W]
    depth = np.stack([1.5 + 3.0 * (0.5 + 0.5 * np.sin(2 * np.pi * (1.3 * uu / W + 0.7 * vv / H + 0.1 * b))) + 0.02 * uu
                      for b in range(B)]).astype(F32)[:, None]
    depth[rng.random(depth.shape) < 0.1] = 0
    if bad and H * W >= 8:
        flat = depth.reshape(B, -1)
        for b in range(B):
            idx = rng.choice(H * W, size=min(4, H * W), replace=False)
            flat[b, idx[0]] = np.nan
            flat[b, idx[1]] = np.inf
            flat[b, idx[2]] = -1.5
            flat[b, idx[3]] = -np.inf
    mask = (rng.random((B, 1, H, W)) >= 0.1).astype(np.uint8)
    if H * W == 1:   # a single pixel: keep it valid, or the case says nothing
        depth[:], mask[:] = 2.5, 1
    return rgb, depth, mask, make_K(B, H, W)
