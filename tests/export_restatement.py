"""NumPy restatement of the inference-export arithmetic (include/cad/cad.h, "inference export"), operation
for operation as specified, plus a PNG reader written from the standard library alone.  Shared by
test_export_cpu.py and test_gpu_export.py; not a test itself.

  lut(name)          the built-in colour tables in Python integers
  ref_range          per image (min, max) over the valid pixels, (0, 0) without one
  ref_colorize       float32: t = (v - lo) / (hi - lo) (subtract, subtract, divide, each rounded to fp32),
                     clamp, idx = rint(t * 255) (half to even), LUT[idx]; hi - lo < 1e-6 -> idx 0
  index_margin       float64 distance of 255 t from the nearest half-integer (the tests' safeguard)
  ref_uint16         float32: rint(d * units) clamped to [0, 65535], 0 where d is not finite or <= 0
  ref_points         float64 unprojection of the valid stride-grid pixels in row-major order
  read_png           signature, IHDR, every chunk CRC, the inflated length, the five scanline filters"""
import struct
import zlib

import numpy as np


# ---------------- colour tables ----------------
def lut(name):
    def c(v):
        return min(255, max(0, v))
    rows = []
    for i in range(256):
        if name == "gray":
            rows.append((i, i, i))
        elif name == "jet":
            rows.append((c(383 - abs(4 * i - 765)), c(383 - abs(4 * i - 510)), c(383 - abs(4 * i - 255))))
        elif name == "hot":
            rows.append((c(8 * i // 3), c(8 * max(i - 96, 0) // 3), c(max(0, 4 * (i - 191) - 1))))
        else:
            raise KeyError(name)
    return np.array(rows, np.uint8)


# ---------------- inputs ----------------
def make_depth(B, H, W, seed=0):
    """depth (B,1,H,W) float32 in (0.3, 9) with NaN, +-inf, zeros and negatives sprinkled in, a second map
    `sub` with zeros, and a uint8 mask with ~15 % zeros."""
    rng = np.random.default_rng(1000 + seed + 7 * B + 31 * H + 131 * W)
    d = rng.uniform(0.3, 9.0, (B, 1, H, W)).astype(np.float32)
    s = (d * np.exp(rng.uniform(-0.4, 0.4, d.shape))).astype(np.float32)
    r = rng.random(d.shape)
    d[r < 0.02] = np.nan
    d[(r >= 0.02) & (r < 0.04)] = np.inf
    d[(r >= 0.04) & (r < 0.05)] = -np.inf
    d[(r >= 0.05) & (r < 0.09)] = 0.0
    d[(r >= 0.09) & (r < 0.12)] = -1.5
    s[rng.random(d.shape) < 0.05] = 0.0
    mask = (rng.random(d.shape) >= 0.15).astype(np.uint8)
    return d, s, mask


def make_camera(B, H, W, seed=0):
    rng = np.random.default_rng(77 + seed)
    K = np.zeros((B, 3, 3), np.float32)
    K[:, 0, 0] = rng.uniform(0.8, 1.3, B) * W
    K[:, 1, 1] = rng.uniform(0.8, 1.3, B) * W
    K[:, 0, 2] = W / 2 + rng.uniform(-3, 3, B)
    K[:, 1, 2] = H / 2 + rng.uniform(-3, 3, B)
    K[:, 2, 2] = 1
    return K


# ---------------- range / render ----------------
def values(depth, sub=None, mask=None):
    """(v, valid) of a batch: v = |d - sub| or d in float32; valid as cad_exporter_range defines it."""
    d = np.asarray(depth, np.float32)
    with np.errstate(all="ignore"):
        v = np.abs(d - np.asarray(sub, np.float32)) if sub is not None else d
        ok = np.isfinite(v) & (d > 0)
        if sub is not None:
            ok &= np.asarray(sub) > 0
    if mask is not None:
        ok &= np.asarray(mask).reshape(d.shape) != 0
    return v, ok


def ref_range(depth, sub=None, mask=None):
    v, ok = values(depth, sub, mask)
    out = np.zeros((v.shape[0], 2), np.float32)
    for b in range(v.shape[0]):
        sel = v[b][ok[b]]
        if sel.size:
            out[b] = sel.min(), sel.max()
    return out


def _t(v, lo, hi):
    f = np.float32
    with np.errstate(all="ignore"):
        return ((v - f(lo)).astype(f) / f(f(hi) - f(lo))).astype(f)


def ref_colorize(depth, table, lo_hi, sub=None, mask=None, invalid=(0, 0, 0)):
    """(B,H,W,3) uint8.  lo_hi: (B,2) per image, or a (lo, hi) pair for all."""
    v, ok = values(depth, sub, mask)
    B, _, H, W = v.shape
    lo_hi = np.broadcast_to(np.asarray(lo_hi, np.float32), (B, 2))
    out = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        lo, hi = lo_hi[b]
        if np.float32(hi - lo) < np.float32(1e-6):
            idx = np.zeros((H, W), np.int64)
        else:
            with np.errstate(all="ignore"):
                t = np.clip(np.nan_to_num(_t(v[b, 0], lo, hi), nan=0.0), np.float32(0), np.float32(1))
                idx = np.rint((t * np.float32(255.0)).astype(np.float32)).astype(np.int64)
        out[b] = table[idx]
        out[b][~ok[b, 0]] = invalid
    return out


def index_margin(depth, lo_hi, sub=None, mask=None):
    """min over the valid pixels of |255 t - (k + 1/2)| in float64 (t clamped); inf for a degenerate range."""
    v, ok = values(depth, sub, mask)
    B = v.shape[0]
    lo_hi = np.broadcast_to(np.asarray(lo_hi, np.float64), (B, 2))
    worst = np.inf
    for b in range(B):
        lo, hi = lo_hi[b]
        sel = v[b][ok[b]].astype(np.float64)
        if hi - lo < 1e-6 or not sel.size:
            continue
        x = 255.0 * np.clip((sel - lo) / (hi - lo), 0.0, 1.0)
        worst = min(worst, np.abs(x - np.floor(x) - 0.5).min())
    return worst


def settle(depth, lo_hi, sub=None, mask=None, margin=1e-3):
    """A copy of depth whose valid pixels keep 255 t away from the half-integers: a pixel within 4 * margin
    of one moves by a quarter of an index step.  Such a pixel is neither the minimum nor the maximum of its
    image (there 255 t is 0 or 255) and stays between them, so the image's range does not change."""
    d = np.array(depth, np.float32)
    v, ok = values(d, sub, mask)
    lo_hi = np.broadcast_to(np.asarray(lo_hi, np.float64), (d.shape[0], 2))
    for b in range(d.shape[0]):
        lo, hi = lo_hi[b]
        if hi - lo < 1e-6:
            continue
        with np.errstate(all="ignore"):
            x = 255.0 * np.clip((v[b].astype(np.float64) - lo) / (hi - lo), 0.0, 1.0)
            bad = ok[b] & (np.abs(x - np.floor(x) - 0.5) < 4 * margin)
        d[b][bad] += np.float32(0.25 / 255.0 * (hi - lo))
    return d


def ref_uint16(depth, units=1000.0):
    d = np.asarray(depth, np.float32)
    with np.errstate(all="ignore"):
        z = np.rint((d * np.float32(units)).astype(np.float32))
        z = np.clip(np.nan_to_num(z, nan=0.0, posinf=65535.0, neginf=0.0), 0, 65535)
    z[~(np.isfinite(d) & (d > 0))] = 0
    return z.astype(np.uint16).reshape(d.shape[0], d.shape[-2], d.shape[-1])


# ---------------- points ----------------
def ref_points(depth, K, rgb=None, mask=None, stride=1, lo=0.1, hi=10.0):
    """Per image: (xyz float64 (N,3), zbits uint32 (N,), rgba uint8 (N,4)) in row-major pixel order."""
    d = np.asarray(depth, np.float32)
    B, _, H, W = d.shape
    out = []
    for b in range(B):
        Z = d[b, 0]
        with np.errstate(all="ignore"):
            ok = np.isfinite(Z) & (Z > np.float32(lo)) & (Z < np.float32(hi))
        if mask is not None:
            ok &= np.asarray(mask)[b].reshape(H, W) != 0
        grid = np.zeros((H, W), bool)
        grid[::stride, ::stride] = True
        ys, xs = np.nonzero(ok & grid)          # row-major
        z = Z[ys, xs]
        fx, fy, cx, cy = (float(K[b, 0, 0]), float(K[b, 1, 1]), float(K[b, 0, 2]), float(K[b, 1, 2]))
        xyz = np.stack([(xs - cx) / fx * z.astype(np.float64), (ys - cy) / fy * z.astype(np.float64), z.astype(np.float64)], 1)
        rgba = np.full((len(z), 4), 255, np.uint8)
        if rgb is not None:
            c = np.asarray(rgb, np.float32)[b][:, ys, xs].T
            rgba[:, :3] = np.rint((np.clip(c, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.float32)).astype(np.uint8)
        out.append((xyz, z.view(np.uint32), rgba))
    return out


# ---------------- PNG, from the standard library ----------------
def read_png(data):
    """The pixels of a non-interlaced 8/16-bit gray or RGB PNG: (H,W) or (H,W,3), uint8 or uint16."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    p, idat, ihdr, seen_end = 8, b"", None, False
    while p < len(data):
        n, typ = struct.unpack(">I4s", data[p:p + 8])
        body = data[p + 8:p + 8 + n]
        crc, = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert zlib.crc32(typ + body) == crc, f"CRC of {typ}"
        if typ == b"IHDR":
            assert p == 8 and n == 13, "IHDR first"
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        elif typ == b"IEND":
            assert n == 0
            seen_end = True
        p += 12 + n
    assert ihdr is not None and seen_end and p == len(data)
    w, h, bits, ctype, comp, filt, interlace = ihdr
    assert w > 0 and h > 0 and bits in (8, 16) and ctype in (0, 2) and comp == 0 and filt == 0 and interlace == 0, ihdr
    ch = 1 if ctype == 0 else 3
    bpp = ch * bits // 8
    stride = w * bpp
    raw = zlib.decompress(idat)
    assert len(raw) == h * (1 + stride), "inflated length"
    img = bytearray(h * stride)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)]
        o = y * stride
        for i in range(stride):
            a = img[o + i - bpp] if i >= bpp else 0
            b = img[o - stride + i] if y else 0
            c = img[o - stride + i - bpp] if (y and i >= bpp) else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) >> 1
            elif ft == 4:
                q = a + b - c
                pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                pred = a if (pa <= pb and pa <= pc) else b if pb <= pc else c
            else:
                raise AssertionError(f"filter type {ft}")
            img[o + i] = (line[i] + pred) & 255
    arr = np.frombuffer(bytes(img), ">u2" if bits == 16 else np.uint8).astype(np.uint16 if bits == 16 else np.uint8)
    return arr.reshape((h, w) if ch == 1 else (h, w, 3))


def read_ply(data):
    """(header text, record bytes) of a PLY file."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode(), data[end:]


def ply_header(n):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "end_header\n" % n)
