"""Restatement of the declared colour augmentation (include/cad/cad.h, cad_sample: saturation / hue matrix and
gamma) for the tests: the matrix in float64 rounded to fp32, the colour step in fp32 numpy in the kernel's
operation order (numpy never fuses a multiply-add, so it is bit-exact against the unfused device code), gamma as
float64 pow rounded to fp32, composed with the oracle's getSample restatement; and the sampler's three extra
draws on top of the oracle's libstdc++ restatement.  A helper module: no tests here."""
import numpy as np
import torch

from oracle import cad_oracle as O

# NTSC RGB -> YIQ
T = np.array([[0.299, 0.587, 0.114], [0.595716, -0.274453, -0.321263], [0.211456, -0.522591, 0.311135]], np.float64)
LUMA = T[0].astype(np.float32)


def color_matrix(saturation, hue):
    """M = T^-1 D T, D = diag(1, s R(2 pi hue)), as I + T^-1 (D - I) T in float64, rounded to fp32."""
    s, th = float(np.float32(saturation)), 2.0 * np.pi * float(np.float32(hue))
    cs, sn = s * np.cos(th), s * np.sin(th)
    E = np.array([[0, 0, 0], [0, cs - 1.0, -sn], [0, sn, cs - 1.0]], np.float64)
    return (np.eye(3) + np.linalg.inv(T) @ E @ T).astype(np.float32)


def apply_color(rgb, M):
    """c' = clamp((M[c][0] r + M[c][1] g) + M[c][2] b, 0, 1), fp32, (3, H, W) numpy."""
    rgb = np.asarray(rgb, np.float32)
    M = np.asarray(M, np.float32)
    r, g, b = rgb[0], rgb[1], rgb[2]
    out = [np.clip((M[c, 0] * r + M[c, 1] * g) + M[c, 2] * b, np.float32(0), np.float32(1)) for c in range(3)]
    out = np.stack(out)
    assert out.dtype == np.float32
    return out


def apply_gamma(rgb, gamma):
    """pow(clamp(v, 0, 1), gamma) in float64, rounded to fp32."""
    v = np.clip(np.asarray(rgb, np.float32), np.float32(0), np.float32(1)).astype(np.float64)
    return np.power(v, float(np.float32(gamma))).astype(np.float32)


def get_sample_declared(rgb_u8_hwc, depth_u16, K, H, W, aug=None, bgr=False, depth_scale=1.0 / 1000.0, M=None):
    """oracle.get_sample with the two declared steps between augmentSample and the second resize.  M: the
    matrix to apply for aug["color"] (default: color_matrix(aug["saturation"], aug["hue"]))."""
    rgb, depth, K = O.load_sample(rgb_u8_hwc, depth_u16, K, bgr, depth_scale)
    rgb, depth, K = O.resize_sample(rgb, depth, K, H, W)
    if aug and aug.get("aug"):
        rgb, depth, K = O.augment_sample(rgb, depth, K, aug)
        x = rgb.contiguous().numpy()
        if aug.get("color"):
            x = apply_color(x, color_matrix(aug["saturation"], aug["hue"]) if M is None else M)
        if aug.get("gamma_on"):
            x = apply_gamma(x, aug["gamma"])
        rgb = torch.from_numpy(np.ascontiguousarray(x))
        rgb, depth, K = O.resize_sample(rgb, depth, K, H, W)
    return rgb, depth, K


class DeclaredDraws(O.StdMt19937Draws):
    """cad_aug_sampler_draw: augmentSample's draws, then saturation, hue, gamma from the same engine."""

    def draw(self, H, W):
        out = super().draw(H, W)
        c = self.cfg
        one = np.float32(1.0)
        out.update(color=0, saturation=1.0, hue=0.0, gamma_on=int(bool(c.get("enable_random_gamma", 0))), gamma=1.0)
        ds, dh = np.float32(c.get("saturation_delta", 0.0)), np.float32(c.get("hue_delta", 0.0))
        if c["enable_color_jitter"] and ds > 0:
            out["saturation"] = float(self._real(one - ds, one + ds))
            out["color"] = 1
        if c["enable_color_jitter"] and dh > 0:
            out["hue"] = float(self._real(-dh, dh))
            out["color"] = 1
        if out["gamma_on"]:
            out["gamma"] = float(self._real(c["gamma_min"], c["gamma_max"]))
        return out
