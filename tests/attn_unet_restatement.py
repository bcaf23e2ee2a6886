"""Restatement of IntrinsicsAttentionUNetImpl (reference src/models/intrinsics_unet.h:278-385) for the
tests of the attention U-Net: a helper, not a test.

Composed from the project's own cad_oracle functions (_double_conv, _convT2x2, _cbam, normalize_cam,
cam_from_K) in the reference's wiring (:339-369): the FiLM U-Net with att<k> = CBAM(f * 2^(k-1)) after
dec<k>, ahead of the 1x1 depth head.  Works in fp32 and in fp64.

bf16 engine (cad_oracle._GEMM["operands"] == "bf16"): operands are rounded as cad_oracle does for
"film" (conv / ConvT operands, stored pre-BN outputs, conv2's input gradient, the bottleneck output's
and the skips' gradients).  The tensors on either side of a CBAM and their gradients stay in the
working dtype: no gradient rounding at a decoder block's output.
"""
import contextlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cad_oracle as O


def attn_param_spec(f, in_ch=3):
    """named_parameters() order (intrinsics_unet.h:311-336): the "film" table through dec1.*, then
    att4.* .. att1.*, then out_conv.*."""
    film = O.param_spec(f, in_ch, model="film")
    spec = film[:-2]
    for k in (4, 3, 2, 1):
        spec += O._cbam_spec(f"att{k}.", f << (k - 1))
    return spec + film[-2:]


def attn_buffer_spec(f, in_ch=3):
    return O.buffer_spec(f, in_ch, model="film")   # CBAM has no buffers


def attn_init(f, seed=0x1A17):
    """Seeded counter-stream weights (cad_oracle.synth_init's rule over attn_param_spec): >= 2-D
    (2u-1)/sqrt(fan_in); BatchNorm weights and fc_gamma biases 1 + 0.1(2u-1); every other 1-D tensor —
    the BatchNorm biases and the CBAM biases among them — 0.1(2u-1): no gradient is trivially zero."""
    params = OrderedDict()
    off = 0
    one, two, tenth = np.float32(1.0), np.float32(2.0), np.float32(0.1)
    for name, shape in attn_param_spec(f):
        n = int(np.prod(shape))
        u = O.u01(seed, np.arange(off, off + n, dtype=np.uint64))
        if len(shape) >= 2:
            v = (two * u - one) * (one / np.sqrt(np.float32(n // shape[0])))
        elif name.endswith(".weight") or name.endswith(".fc_gamma.bias"):
            v = one + tenth * (two * u - one)
        else:
            v = tenth * (two * u - one)
        params[name] = torch.from_numpy(v.astype(np.float32).reshape(shape))
        off += n
    return params


def attn_init_buffers(f):
    return OrderedDict((n, torch.zeros(s) if n.endswith("mean") else torch.ones(s)) for n, s in attn_buffer_spec(f))


@contextlib.contextmanager
def _single_value_batchnorm():
    """torch.nn.functional.batch_norm refuses a train-mode batch with one value per channel (B = 1 at a
    1x1 bottleneck).  The check is Python's alone: LibTorch's BatchNorm2d, which the reference runs,
    normalises such a batch (x_hat = 0, output = bias) and updates running_var with the unbiased variance
    0 / 0 = NaN.  The guard is lifted while the restatement runs, so that it does what the reference does."""
    prev = F._verify_batch_size
    F._verify_batch_size = lambda size: None
    try:
        yield
    finally:
        F._verify_batch_size = prev


def attn_unet_forward(x, p, bufs, train=True, max_depth=10.0, K=None, keep=None):
    """IntrinsicsAttentionUNetImpl::forward(x, cam_from_K(K)).  keep (dict): receives the input of every
    att<k> as "z<k>"."""
    with _single_value_batchnorm():
        return _forward(x, p, bufs, train, max_depth, K, keep)


def _forward(x, p, bufs, train, max_depth, K, keep):
    cam = O.normalize_cam(O.cam_from_K(K.to(x.dtype)), x.shape[3], x.shape[2])
    r = p["enc1.conv1.weight"].shape[0] % 8 == 0       # the pre-split path needs f % 8 == 0
    rb = r and O._GEMM["operands"] == "bf16"
    pool = lambda t: F.max_pool2d(O._RoundOperand.apply(t) if rb else t, 2)
    s1 = O._double_conv(x, p, bufs, "enc1.", train, cam, r)
    s2 = O._double_conv(pool(s1), p, bufs, "enc2.conv.", train, cam, r)
    s3 = O._double_conv(pool(s2), p, bufs, "enc3.conv.", train, cam, r)
    s4 = O._double_conv(pool(s3), p, bufs, "enc4.conv.", train, cam, r)
    x = O._double_conv(pool(s4), p, bufs, "bottleneck.conv.", train, cam, r)
    if rb:   # dec4's ConvT input gradient (the bottleneck output's) is stored as bf16
        x = O._RoundGradOperand.apply(x)
    for k, skip in ((4, s4), (3, s3), (2, s2), (1, s1)):
        pre = f"dec{k}."
        # FiLMDecoderBlockImpl::forward (:91-110): up, cat({skip, up}), conv
        u = O._convT2x2(x, p[pre + "up.weight"], p[pre + "up.bias"], r)
        if rb:   # the skip half of the concat's gradient is stored as bf16
            skip = O._RoundGradOperand.apply(skip)
        z = O._double_conv(torch.cat([skip, u], 1), p, bufs, pre + "conv.", train, cam, r)
        if keep is not None:
            keep[f"z{k}"] = z
        x = O._cbam(z, p, f"att{k}.")
    x = F.conv2d(x, p["out_conv.weight"], p["out_conv.bias"])
    return torch.sigmoid(x) * max_depth


def level0(y, scale, shift, p, pre, w, b, max_depth):
    """The restated level 0: bn-affine -> relu -> _cbam -> 1x1 -> sigmoid * md.  y (B,C,H,W); returns
    (z, pred)."""
    z = F.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    out = O._cbam(z, p, pre)
    logit = F.conv2d(out, w.view(1, -1, 1, 1), b.view(1))
    return z, torch.sigmoid(logit) * max_depth


class AttnTrainer(O.Trainer):
    """cad_oracle.Trainer (one replica of the reference's train step) around attn_unet_forward."""

    def __init__(self, params, buffers, **kw):
        kw.pop("model", None)
        super().__init__(params, buffers, model="film", **kw)

    def forward_backward(self, rgb, gt, K):
        rgb, gt, K = (t.to(self.device, self.dtype) for t in (rgb, gt, K))
        for v in self.p.values():
            v.requires_grad_(True)
            v.grad = None
        prev, O._GEMM["operands"] = O._GEMM["operands"], self.gemm_operands
        try:
            pred = attn_unet_forward(rgb, self.p, self.bufs, True, self.max_depth, K)
            pred.retain_grad()
            loss, comps = O.combined_loss(pred, gt, rgb, K, self.weights)
            loss.sum().backward()
        finally:
            O._GEMM["operands"] = prev
        grads = [v.grad.detach().clone() if v.grad is not None else None for v in self.p.values()]
        for v in self.p.values():
            v.requires_grad_(False)
        return pred.detach(), pred.grad.detach(), float(loss.detach()), comps, grads

    @torch.no_grad()
    def predict_eval(self, rgb, K=None, keep=None):
        prev, O._GEMM["operands"] = O._GEMM["operands"], self.gemm_operands
        try:
            return attn_unet_forward(rgb.to(self.device, self.dtype), self.p, self.bufs, False, self.max_depth,
                                     K.to(self.device, self.dtype), keep)
        finally:
            O._GEMM["operands"] = prev
