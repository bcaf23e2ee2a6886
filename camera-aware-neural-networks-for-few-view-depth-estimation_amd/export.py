"""Inference and export (the "inference export" section of include/cad/cad.h): one image in, a depth map
out, and the files a depth map is exchanged as.

  Predictor                eval-mode forward of any model family (+ flip test-time augmentation), colourised
                           renders, 16-bit depth and point clouds on the device (cad_exporter_*,
                           csrc/kernels/export_kernels.hip; the reference's DepthVisualizer,
                           src/visualization/depth_viz.h:23-148)
  save_png / load_png      cad_png_encode / cad_png_decode (8/16-bit gray or RGB), host only
  save_ply                 cad_ply_write of the point records, host only
  colormap_lut             the built-in 256 x 3 colour tables, host only

torch is device-memory plumbing here as everywhere: every computation runs in the HIP kernels."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import check


def colormap_lut(name: str) -> np.ndarray:
    """(256, 3) uint8 table of "gray", "jet" or "hot" (CadError for another name)."""
    out = np.empty((256, 3), np.uint8)
    check(_abi.load().cad_colormap_lut(str(name).encode(), out.ctypes.data), "cad_colormap_lut")
    return out


def encode_png(pixels: np.ndarray) -> bytes:
    """A uint8 / uint16 array (H,W), (H,W,1) or (H,W,3) as the bytes of a PNG file."""
    a = np.ascontiguousarray(pixels)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3):
        raise ValueError("PNG pixels must be a uint8 or uint16 array of shape (H,W) or (H,W,C)")
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    lib = _abi.load()
    size = C.c_int64()
    bits = 8 * a.dtype.itemsize
    check(lib.cad_png_encode(a.ctypes.data, h, w, ch, bits, None, 0, C.byref(size)), "cad_png_encode")
    buf = np.empty(size.value, np.uint8)
    check(lib.cad_png_encode(a.ctypes.data, h, w, ch, bits, buf.ctypes.data, buf.size, C.byref(size)), "cad_png_encode")
    return buf[:size.value].tobytes()


def decode_png(data: bytes) -> np.ndarray:
    """The pixels of a PNG file held in memory: (H,W) for one channel, else (H,W,C); uint8 or uint16."""
    lib = _abi.load()
    src = np.frombuffer(data, np.uint8)
    h, w, ch, bits = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    dims = (C.byref(h), C.byref(w), C.byref(ch), C.byref(bits))
    check(lib.cad_png_decode(src.ctypes.data, src.size, None, 0, *dims), "cad_png_decode")
    out = np.empty((h.value, w.value, ch.value), np.uint16 if bits.value == 16 else np.uint8)
    check(lib.cad_png_decode(src.ctypes.data, src.size, out.ctypes.data, out.nbytes, *dims), "cad_png_decode")
    return out[:, :, 0] if ch.value == 1 else out


def save_png(path, pixels: np.ndarray) -> None:
    with open(path, "wb") as fh:
        fh.write(encode_png(pixels))


def load_png(path) -> np.ndarray:
    with open(path, "rb") as fh:
        return decode_png(fh.read())


POINT_DTYPE = np.dtype([("xyz", np.float32, 3), ("rgba", np.uint8, 4)])   # one 16-byte record


def save_ply(path, xyz, rgba=None) -> None:
    """A binary little-endian PLY of n points: xyz (n,3) float32 and rgba (n,4) uint8 (white without it), or
    a record array of POINT_DTYPE as Predictor.points holds them."""
    if rgba is None and getattr(xyz, "dtype", None) == POINT_DTYPE:
        rec = np.ascontiguousarray(xyz)
    else:
        xyz = np.asarray(xyz.cpu() if hasattr(xyz, "cpu") else xyz, np.float32).reshape(-1, 3)
        rec = np.empty(len(xyz), POINT_DTYPE)
        rec["xyz"] = xyz
        rec["rgba"] = 255 if rgba is None else np.asarray(rgba.cpu() if hasattr(rgba, "cpu") else rgba, np.uint8).reshape(-1, 4)
    check(_abi.load().cad_ply_write(str(path).encode(), rec.ctypes.data, len(rec)), "cad_ply_write")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Predictor:
    """Predictor(model, batch, height, width): inference with a trained model and export of its depth maps.

    model may be None for an exporter without a network (colorize / to_uint16 / points of any depth map of
    that size).  Every method enqueues on the current stream; nothing is copied to the host."""

    def __init__(self, model, batch: int, height: int, width: int, device: int | None = None, fused_eval=None):
        """fused_eval (None: leave the model's switch): predict with the fused eval forward (model.fused_eval)."""
        import torch
        self.lib = _abi.load()
        if model is not None:
            from . import model as M
            M._set_fused_eval(model, fused_eval)
        self.model, self.batch, self.height, self.width = model, int(batch), int(height), int(width)
        dev = device if device is not None else (model.device.index if model is not None else 0)
        self.device = torch.device("cuda", dev or 0)
        h = C.c_void_p()
        check(self.lib.cad_exporter_create(self.batch, self.height, self.width, self.device.index, C.byref(h)),
              "cad_exporter_create")
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.cad_exporter_destroy(h)
            self.h = None

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _f32(self, t, shape_tail, what):
        import torch
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f"{what}: contiguous fp32 device tensor"
        assert tuple(t.shape[-len(shape_tail):]) == shape_tail, f"{what}: expected (..., {shape_tail}), got {tuple(t.shape)}"
        return t

    def _depth(self, depth, what="depth"):
        d = self._f32(depth, (self.height, self.width), what)
        B = d.numel() // (self.height * self.width)
        assert 1 <= B <= self.batch, f"{what}: batch {B} exceeds the predictor's {self.batch}"
        return d, B

    def _mask(self, mask, like):
        import torch
        if mask is None:
            return None
        assert mask.numel() == like.numel(), "mask must match the depth map"
        return mask if mask.dtype == torch.uint8 and mask.is_contiguous() else mask.to(torch.uint8).contiguous()

    # ---- inference ----
    def predict(self, rgb, K=None, flip_tta: bool = False):
        """Depth (B,1,H,W) of rgb (B,3,H,W) by the model's eval-mode forward; its train / eval mode is restored.
        K (B,3,3) is required by the conditioned and geometry models.  flip_tta: the mean of f(x, K) and the
        mirrored f(hflip(x), K'), K' = K with cx' = W - 1 - cx (applyHorizontalFlip)."""
        from . import model as M
        m = self.model
        if m is None:
            raise ValueError("Predictor.predict needs a model")
        needs_K = isinstance(m, M.GeometryAwareNetwork) or getattr(m, "conditioned", False)
        if needs_K and K is None:
            raise ValueError("this model is conditioned on the camera: predict needs K (B,3,3)")
        was_training = bool(getattr(m, "training", True))
        m.eval()
        try:
            pred = M._eval_forward(m, rgb, K)
            if flip_tta:
                Kf = None
                if K is not None:
                    Kf = K.clone()
                    Kf[:, 0, 2] = (self.width - 1) - K[:, 0, 2]
                pf = M._eval_forward(m, self.hflip(rgb), Kf)
                pred = self.flip_mean(pred, pf, out=pred)
        finally:
            m.train(was_training)
        return pred

    def hflip(self, x):
        """x (..., H, W) mirrored left to right."""
        import torch
        x = self._f32(x, (self.height, self.width), "hflip")
        out = torch.empty_like(x)
        planes = x.numel() // (self.height * self.width)
        check(self.lib.cad_hflip(_p(x), _p(out), planes, self.height, self.width, self._stream()), "cad_hflip")
        return out

    def flip_mean(self, a, b, out=None):
        """0.5 * (a + hflip(b)); out may be a."""
        import torch
        a = self._f32(a, (self.height, self.width), "flip_mean")
        b = self._f32(b, (self.height, self.width), "flip_mean")
        assert a.shape == b.shape
        if out is None:
            out = torch.empty_like(a)
        planes = a.numel() // (self.height * self.width)
        check(self.lib.cad_flip_mean(_p(a), _p(b), _p(out), planes, self.height, self.width, self._stream()), "cad_flip_mean")
        return out

    # ---- export ----
    def depth_range(self, depth, mask=None, sub=None):
        """(B,2) device tensor (min, max) of depth (|depth - sub| with sub) over each image's valid pixels:
        finite, depth > 0 (sub > 0), mask != 0; (0, 0) without one."""
        import torch
        d, B = self._depth(depth)
        if sub is not None:
            self._depth(sub, "sub")
        m = self._mask(mask, d)
        out = torch.empty((B, 2), dtype=torch.float32, device=self.device)
        check(self.lib.cad_exporter_range(self.h, _p(d), _p(sub), _p(m), B, _p(out), self._stream()), "cad_exporter_range")
        return out

    def _opts(self, colormap="jet", vmin=None, vmax=None, invalid=(0, 0, 0), row_stride=0, col_offset=0, image_stride=0,
              units_per_metre=1000.0):
        o = _abi.RenderOpts()
        if isinstance(colormap, str):
            if colormap not in _abi.COLORMAPS:
                raise ValueError(f"colormap must be one of {tuple(_abi.COLORMAPS)} or a (256,3) uint8 table, not {colormap!r}")
            o.colormap = _abi.COLORMAPS[colormap]
        else:
            lut = np.ascontiguousarray(colormap, np.uint8)
            if lut.size != 768:
                raise ValueError("a colour table holds 256 x 3 bytes")
            check(self.lib.cad_exporter_set_lut(self.h, lut.ctypes.data), "cad_exporter_set_lut")
            o.colormap = _abi.CMAP_CUSTOM
        if (vmin is None) != (vmax is None):
            raise ValueError("give both vmin and vmax, or neither")
        o.fixed_range = int(vmin is not None)
        o.lo, o.hi = (float(vmin), float(vmax)) if vmin is not None else (0.0, 0.0)
        o.invalid[:] = [int(c) for c in invalid]
        o.row_stride, o.col_offset, o.image_stride = int(row_stride), int(col_offset), int(image_stride)
        o.units_per_metre = float(units_per_metre)
        return o

    def colorize(self, depth, colormap="jet", vmin=None, vmax=None, mask=None, sub=None, invalid=(0, 0, 0), out=None,
                 col_offset=0):
        """(B,H,W,3) uint8 on the device: LUT[rint(255 * clamp((v - lo) / (hi - lo)))], v = depth (|depth - sub|
        with sub), lo / hi = vmin / vmax or each image's own valid range; invalid pixels get `invalid`.
        out: a (B,H,Wp,3) uint8 panel whose columns col_offset .. col_offset + W - 1 receive the pane."""
        import torch
        d, B = self._depth(depth)
        if sub is not None:
            self._depth(sub, "sub")
        m = self._mask(mask, d)
        row = 0
        if out is None:
            out = torch.empty((B, self.height, self.width, 3), dtype=torch.uint8, device=self.device)
        else:
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 4
            assert out.shape[0] >= B and out.shape[1] == self.height and out.shape[3] == 3
            row = out.shape[2]
        o = self._opts(colormap, vmin, vmax, invalid, row_stride=row, col_offset=col_offset)
        if not o.fixed_range:
            check(self.lib.cad_exporter_range(self.h, _p(d), _p(sub), _p(m), B, None, self._stream()), "cad_exporter_range")
        check(self.lib.cad_exporter_render(self.h, _p(d), _p(sub), _p(m), B, C.byref(o), _p(out), None, self._stream()),
              "cad_exporter_render")
        return out

    def image_pane(self, rgb, out, col_offset=0):
        """rgb (B,3,H,W) in [0,1] as an RGB8 pane of the panel `out` (B,H,Wp,3) uint8."""
        r = self._f32(rgb, (3, self.height, self.width), "rgb")
        o = self._opts(row_stride=out.shape[2], col_offset=col_offset)
        check(self.lib.cad_exporter_image(self.h, _p(r), r.shape[0], C.byref(o), _p(out), self._stream()), "cad_exporter_image")
        return out

    def normals(self, depth, K, mask=None, invalid=(0, 0, 0), out=None, col_offset=0):
        """(B,H,W,3) uint8 on the device: the surface normals of depth (B,1,H,W) from K (B,3,3), coloured
        rint(255 * ((n_x + 1) / 2, (1 - n_y) / 2, (1 - n_z) / 2)), a frontal wall (128, 128, 255).  Pixels whose
        own or neighbouring depth is invalid (not finite, <= 0, mask == 0), the border included, get `invalid`.
        out / col_offset as in colorize."""
        import torch
        d, B = self._depth(depth)
        Kc = self._f32(K, (3, 3), "K")
        assert Kc.numel() == 9 * B, "K must be (B,3,3)"
        m = self._mask(mask, d)
        row = 0
        if out is None:
            out = torch.empty((B, self.height, self.width, 3), dtype=torch.uint8, device=self.device)
        else:
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 4
            assert out.shape[0] >= B and out.shape[1] == self.height and out.shape[3] == 3
            row = out.shape[2]
        o = self._opts(invalid=invalid, row_stride=row, col_offset=col_offset)
        check(self.lib.cad_exporter_normals(self.h, _p(d), _p(Kc), _p(m), B, C.byref(o), _p(out), self._stream()),
              "cad_exporter_normals")
        return out

    def to_uint16(self, depth, units_per_metre: float = 1000.0):
        """(B,H,W) uint16 on the device: rint(depth * units_per_metre) clamped to 65535; 0 where the depth is
        not finite or not positive (1000: SUN RGB-D's millimetre PNGs)."""
        import torch
        d, B = self._depth(depth)
        out = torch.empty((B, self.height, self.width), dtype=torch.uint16, device=self.device)
        o = self._opts(units_per_metre=units_per_metre)
        check(self.lib.cad_exporter_render(self.h, _p(d), None, None, B, C.byref(o), None, _p(out), self._stream()),
              "cad_exporter_render")
        return out

    def points_raw(self, depth, K, rgb=None, mask=None, stride=1, min_depth=0.1, max_depth=10.0, out=None):
        """The record buffer (B, cap, 16) uint8 and the counts (B,) int32, both on the device, without a
        host synchronisation; cap = ceil(H/stride) * ceil(W/stride)."""
        import torch
        d, B = self._depth(depth)
        stride = int(stride)
        cap = -(-self.height // stride) * -(-self.width // stride) if stride >= 1 else 1
        Kc = self._f32(K, (3, 3), "K")
        assert Kc.numel() == 9 * B, "K must be (B,3,3)"
        if rgb is not None:
            self._f32(rgb, (3, self.height, self.width), "rgb")
        m = self._mask(mask, d)
        if out is None:
            out = (torch.empty((B, cap, 16), dtype=torch.uint8, device=self.device),
                   torch.empty((B,), dtype=torch.int32, device=self.device))
        rec, cnt = out
        check(self.lib.cad_exporter_points(self.h, _p(d), _p(Kc), _p(rgb), _p(m), B, stride, float(min_depth),
                                           float(max_depth), _p(rec), _p(cnt), self._stream()), "cad_exporter_points")
        return rec, cnt

    def points(self, depth, K, rgb=None, mask=None, stride=1, min_depth=0.1, max_depth=10.0):
        """Per image (xyz (N,3) float32, rgba (N,4) uint8): views of the device record buffer, in row-major
        pixel order.  Reads the counts back (one synchronisation)."""
        import torch
        rec, cnt = self.points_raw(depth, K, rgb, mask, stride, min_depth, max_depth)
        out = []
        for b, n in enumerate(cnt.cpu().tolist()):
            r = rec[b, :n]
            out.append((r[:, :12].view(torch.float32), r[:, 12:]))
        return out
