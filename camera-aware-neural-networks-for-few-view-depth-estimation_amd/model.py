"""Python host mirror of the reference's hot-path operator API, on libcad_hip.so.

Class and method names follow the reference so that a caller (and the parity tests) read like
the reference's own code:

  BaselineUNet            BaselineUNetImpl           src/models/baseline_unet.h:122-208
  IntrinsicsConditionedUNet IntrinsicsConditionedUNetImpl src/models/intrinsics_unet.h:137-270
  IntrinsicsAttentionUNet IntrinsicsAttentionUNetImpl src/models/intrinsics_unet.h:278-385
  RayConditionedUNet      config-3 composite: enc1 = RayEnhancedConv (geometry_aware_network.h:17-65),
                          FiLM blocks after (intrinsics_unet.h:16-113)
  CombinedDepthLoss       CombinedDepthLoss          src/loss/depth_loss.h:366-479
  Adam                    torch::optim::Adam         (options built at tensorboard_trainer_enhanced.h:97-101)
  Optimizer               torch::optim::Adam / AdamW / SGD by rule (src/training/trainer.h:388-414), with an
                          optional EMA of the weights kept in the same pass (no reference counterpart)
  clip_grad_norm_         torch::nn::utils::clip_grad_norm_ (enhanced.h:300-302)
  Trainer.train_step      TensorBoardTrainerEnhanced::trainEpoch body, enhanced.h:287-304

torch is used only as device-memory / stream / torch.distributed plumbing: every computation on the
path runs in the HIP kernels behind the C ABI.  Tensors are torch CUDA (HIP) tensors in the
reference's NCHW fp32 layout.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _abi
from ._abi import check


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: torch.Tensor):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32, "expected contiguous fp32 device tensor"
    return C.c_void_p(t.data_ptr())


MODEL_BASELINE, MODEL_INTRINSICS_FILM, MODEL_RAY_FILM, MODEL_INTRINSICS_ATTN = 0, 1, 2, 3   # CAD_MODEL_* of cad.h


def _histograms(model, fn, which):
    """TensorBoard histograms of every parameter ("params") or gradient ("grads") tensor from one device pass
    over the model's flat slab (cad_*_histograms): name -> (stats, counts) in named_parameters() order, stats a
    dict of _abi.HIST_STATS, counts the uint32 array of the _abi.HIST_BINS default buckets."""
    if which not in ("params", "grads"):
        raise ValueError(f"which must be 'params' or 'grads', not {which!r}")
    hh = C.c_void_p()
    check(fn(model.h, 0 if which == "params" else 1, _stream(model.device), C.byref(hh)), "histograms")
    n = len(model._param_info)
    stats = np.empty((n, len(_abi.HIST_STATS)), np.float64)
    counts = np.empty((n, _abi.HIST_BINS), np.uint32)
    check(model.lib.cad_hist_read(hh, stats.ctypes.data_as(_abi.DP), counts.ctypes.data_as(C.POINTER(C.c_uint32))),
          "cad_hist_read")
    return OrderedDict((name, (dict(zip(_abi.HIST_STATS, stats[i].tolist())), counts[i]))
                       for i, (name, _) in enumerate(model._param_info))


class BaselineUNet:
    """BaselineUNetImpl(in_channels, init_features, max_depth) on MI355X.

    Extra keyword-only arguments size the device workspace (the reference allocates per call)."""

    MODEL = MODEL_BASELINE

    def __init__(self, in_channels=3, init_features=64, max_depth=10.0, *, batch, height, width, device=0):
        self.lib = _abi.load()
        self.device = torch.device("cuda", device)
        self.in_channels, self.init_features, self.max_depth = in_channels, init_features, max_depth
        self.batch, self.height, self.width = batch, height, width
        desc = _abi.UnetDesc(in_channels, init_features, max_depth, batch, height, width)
        h = C.c_void_p()
        check(self.lib.cad_unet_create_model(C.byref(desc), self.MODEL, device, C.byref(h)), "cad_unet_create_model")
        self.h = h
        self._param_info = [self._info(0, i) for i in range(self.lib.cad_unet_num_params(h))]
        self._buffer_info = [self._info(1, i) for i in range(self.lib.cad_unet_num_buffers(h))]
        n = C.c_int64()
        check(self.lib.cad_unet_flat(h, None, None, C.byref(n)), "cad_unet_flat")
        self.n_flat = n.value
        # flat slabs owned by torch so torch.distributed (RCCL) can all-reduce them in place
        self.flat_params = torch.zeros(self.n_flat, dtype=torch.float32, device=self.device)
        self.flat_grads = torch.zeros(self.n_flat, dtype=torch.float32, device=self.device)
        check(self.lib.cad_unet_use_external_slabs(h, _ptr(self.flat_params), _ptr(self.flat_grads)),
              "cad_unet_use_external_slabs")
        self.num_stages = self.lib.cad_unet_num_stages(h)
        self.stage_ranges = []
        for s in range(self.num_stages):
            off, cnt = C.c_int64(), C.c_int64()
            check(self.lib.cad_unet_stage_grad_range(h, s, C.byref(off), C.byref(cnt)), "stage range")
            self.stage_ranges.append((off.value, cnt.value))
        self.training = True
        self._out = None

    def _info(self, kind, idx):
        name = C.c_char_p()
        nd = C.c_int()
        shape = (C.c_int64 * 4)()
        check(self.lib.cad_unet_tensor_info(self.h, kind, idx, C.byref(name), C.byref(nd), shape), "tensor_info")
        return name.value.decode(), tuple(shape[i] for i in range(nd.value))

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.cad_unet_destroy(h)
            self.h = None

    # ---- torch::nn::Module surface used by the trainer ----
    def train(self, mode=True):
        self.training = bool(mode)
        check(self.lib.cad_unet_train(self.h, int(mode)), "cad_unet_train")
        return self

    def eval(self):
        return self.train(False)

    def fused_eval(self, on=True):
        """Fused eval forward (cad_unet_set_fused_eval; off by default): eval-mode forwards apply each block's
        BatchNorm + ReLU (+ FiLM) in the 3 x 3 convolutions' epilogues, so the pre-BN outputs are never written.
        Train-mode forwards ignore it.  fp32 engines: the same bits; bf16 engine: one rounding instead of two."""
        check(self.lib.cad_unet_set_fused_eval(self.h, int(bool(on))), "cad_unet_set_fused_eval")
        return self

    def fused_eval_on(self) -> bool:
        return bool(self.lib.cad_unet_get_fused_eval(self.h))

    def fused_eval_convs(self):
        """(fused, total): how many of the last forward's 3 x 3 convolutions ran the fused epilogue."""
        a, b = C.c_int(), C.c_int()
        check(self.lib.cad_unet_fused_eval_convs(self.h, C.byref(a), C.byref(b)), "cad_unet_fused_eval_convs")
        return a.value, b.value

    def count_parameters(self) -> int:
        return int(self.lib.cad_unet_count_parameters(self.h))

    def _get(self, kind, idx, shape):
        out = np.empty(int(np.prod(shape)) if shape else 1, np.float32)
        check(self.lib.cad_unet_get_tensor(self.h, kind, idx, out.ctypes.data_as(_abi.FP), out.size), "get_tensor")
        return torch.from_numpy(out.reshape(shape))

    def named_parameters(self):
        torch.cuda.synchronize(self.device)
        return OrderedDict((n, self._get(0, i, s)) for i, (n, s) in enumerate(self._param_info))

    def named_buffers(self):
        torch.cuda.synchronize(self.device)
        return OrderedDict((n, self._get(1, i, s)) for i, (n, s) in enumerate(self._buffer_info))

    def state_dict(self):
        d = self.named_parameters()
        d.update(self.named_buffers())
        return d

    def load_state_dict(self, state, strict=True):
        torch.cuda.synchronize(self.device)
        names = {n: (0, i, s) for i, (n, s) in enumerate(self._param_info)}
        names.update({n: (1, i, s) for i, (n, s) in enumerate(self._buffer_info)})
        missing = [n for n in names if n not in state]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:5]}")
        for n, (kind, i, s) in names.items():
            if n not in state:
                continue
            v = np.ascontiguousarray(torch.as_tensor(state[n]).detach().cpu().float().numpy())
            assert tuple(v.shape) == tuple(s), f"{n}: shape {v.shape} != {s}"
            check(self.lib.cad_unet_set_tensor(self.h, kind, i, v.ctypes.data_as(_abi.FP), v.size), f"set {n}")

    def grads(self):
        torch.cuda.synchronize(self.device)
        out = OrderedDict()
        for i, (n, s) in enumerate(self._param_info):
            g = np.empty(int(np.prod(s)), np.float32)
            check(self.lib.cad_unet_get_grad(self.h, i, g.ctypes.data_as(_abi.FP), g.size), "get_grad")
            out[n] = torch.from_numpy(g.reshape(s))
        return out

    # ---- forward / backward ----
    @property
    def conditioned(self) -> bool:
        return self.MODEL != MODEL_BASELINE

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        B, Cc, H, W = x.shape
        assert Cc == self.in_channels and H == self.height and W == self.width, "input shape mismatch"
        if out is None:
            out = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        check(self.lib.cad_unet_forward(self.h, _ptr(x), _ptr(out), B, _stream(self.device)), "cad_unet_forward")
        return out

    def forward_cam(self, x: torch.Tensor, intrinsics: torch.Tensor, out: torch.Tensor | None = None):
        """forward(x, camera_intrinsics (B,4) [fx, fy, cx, cy]) of the camera-conditioned models."""
        B, Cc, H, W = x.shape
        assert Cc == self.in_channels and H == self.height and W == self.width, "input shape mismatch"
        assert tuple(intrinsics.shape) == (B, 4), "intrinsics must be (B, 4) [fx, fy, cx, cy]"
        if out is None:
            out = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        check(self.lib.cad_unet_forward_cam(self.h, _ptr(x), _ptr(intrinsics.contiguous()), _ptr(out), B,
                                            _stream(self.device)), "cad_unet_forward_cam")
        return out

    def __call__(self, x, *args, **kw):
        return self.forward_cam(x, *args, **kw) if self.conditioned else self.forward(x, *args, **kw)

    def backward(self, ddepth: torch.Tensor, on_stage=None):
        """Backward of the last train-mode forward. on_stage(stage, offset, count) is called after
        each stage is enqueued (gradients of flat_grads[offset:offset+count] are then final on the
        stream) — the hook the data-parallel trainer uses to overlap RCCL all-reduce."""
        st = _stream(self.device)
        if on_stage is None:
            check(self.lib.cad_unet_backward(self.h, _ptr(ddepth), st), "cad_unet_backward")
            return
        for s in range(self.num_stages):
            check(self.lib.cad_unet_backward_stage(self.h, s, _ptr(ddepth), st), f"backward stage {s}")
            on_stage(s, *self.stage_ranges[s])

    def debug_buffer(self, name: str) -> torch.Tensor:
        """Host copy of an internal NHWC buffer (flat) — debugging / layer-level parity only."""
        n = self.lib.cad_unet_debug_buffer(self.h, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, np.float32)
        assert self.lib.cad_unet_debug_buffer(self.h, name.encode(), out.ctypes.data_as(_abi.FP), n) == n
        return torch.from_numpy(out)

    def num_batches_tracked(self) -> int:
        return int(self.lib.cad_unet_num_batches_tracked(self.h))

    def histograms(self, which="params") -> "OrderedDict[str, tuple]":
        """name -> (stats, counts) of every parameter ("params") or gradient ("grads") tensor: _histograms."""
        return _histograms(self, self.lib.cad_unet_histograms, which)

    def last_grad_norm(self) -> float:
        v = C.c_float()
        check(self.lib.cad_unet_last_grad_norm(self.h, C.byref(v), _stream(self.device)), "last_grad_norm")
        return float(v.value)


def save(model: BaselineUNet, path: str):
    """torch::save(model_, path) (tensorboard_trainer_enhanced.h:656-662): the TorchScript archive
    LibTorch writes for the module, readable by the reference's torch::load (cad_unet_save_torch)."""
    check(model.lib.cad_unet_save_torch(model.h, str(path).encode()), "cad_unet_save_torch")


def load(model: BaselineUNet, path: str):
    """torch::load(model, path): parameters, BatchNorm buffers and num_batches_tracked from a
    torch::save archive (the reference's or ours); every model tensor must be present with its shape."""
    torch.cuda.synchronize(model.device)
    check(model.lib.cad_unet_load_torch(model.h, str(path).encode()), "cad_unet_load_torch")


class IntrinsicsConditionedUNet(BaselineUNet):
    """IntrinsicsConditionedUNetImpl(in_channels, init_features, camera_dim=4, max_depth) on MI355X:
    a FiLMLayerImpl(4, C) after the first BN-ReLU of every DoubleConv, fed the normalised (B,4)
    intrinsics (intrinsics_unet.h:137-270).  forward(x, intrinsics) takes [fx, fy, cx, cy]."""

    MODEL = MODEL_INTRINSICS_FILM

    def __init__(self, in_channels=3, init_features=64, camera_dim=4, max_depth=10.0, *, batch, height, width,
                 device=0):
        assert camera_dim == 4, "camera_dim 4 ([fx, fy, cx, cy]) is the configuration on the hot path"
        super().__init__(in_channels, init_features, max_depth, batch=batch, height=height, width=width,
                         device=device)

    def forward(self, x, intrinsics, out=None):   # noqa: D401 (reference signature)
        return self.forward_cam(x, intrinsics, out)


class IntrinsicsAttentionUNet(IntrinsicsConditionedUNet):
    """IntrinsicsAttentionUNetImpl(in_channels, init_features, camera_dim=4, max_depth) on MI355X: the FiLM
    U-Net with a CBAM (att4 .. att1, spatial_attention.h:142-191) after every decoder block, ahead of the
    1x1 depth head (intrinsics_unet.h:278-385).  Level 0 runs as the fused attention head when
    init_features / 4 is a power of two <= 32."""

    MODEL = MODEL_INTRINSICS_ATTN

    def _int_buffer(self, name):
        return self.debug_buffer(name).view(torch.int32)

    def attention_maps(self, level):
        """CBAMImpl::getAttentionMaps of att<level> (1..4) for the last forward:
        (channel_att [B, C], spatial_att [B, 1, H_l, W_l]) as host tensors."""
        if level not in (1, 2, 3, 4):
            raise ValueError(f"level must be 1..4 (att1 .. att4), not {level!r}")
        l = level - 1
        C_l = self.init_features << l
        att = self.debug_buffer(f"att{l}").view(-1, C_l)
        sa = self.debug_buffer(f"sa{l}").view(att.shape[0], 1, self.height >> l, self.width >> l)
        return att, sa

    def attention_decisions(self, level):
        """The two argmax decisions of att<level>'s last forward: (argmax pixel of the channel max-pool
        [B, C], argmax channel of the spatial max [B, H_l, W_l]), int64 host tensors."""
        l = level - 1
        C_l = self.init_features << l
        amax = self._int_buffer(f"amax{l}").view(-1, C_l).long()
        sidx = self._int_buffer(f"sidx{l}").view(amax.shape[0], self.height >> l, self.width >> l).long()
        return amax, sidx


class RayConditionedUNet(IntrinsicsConditionedUNet):
    """Config-3 model (SURVEY §8 "Recommended config-3 model"): enc1 = RayEnhancedConv(3, f, 4,
    use_rays=true) fed cat(rgb, per-pixel rays from the intrinsics), FiLM blocks after."""

    MODEL = MODEL_RAY_FILM


def camera_from_K(K: torch.Tensor) -> torch.Tensor:
    """(B,3,3) intrinsics -> (B,4) [fx, fy, cx, cy] on device."""
    B = K.shape[0]
    lib = _abi.load()
    out = torch.empty((B, 4), dtype=torch.float32, device=K.device)
    check(lib.cad_camera_from_K(_ptr(K.reshape(B, 9).contiguous()), B, _ptr(out), _stream(K.device)), "camera_from_K")
    return out


def clip_grad_norm_(model: BaselineUNet, max_norm: float, prescale: float = 1.0):
    """torch::nn::utils::clip_grad_norm_ over all parameters (device-resident total norm)."""
    check(model.lib.cad_clip_grad_norm(model.h, float(max_norm), float(prescale), _stream(model.device)), "clip")


class Adam:
    """torch::optim::Adam(params, AdamOptions(lr).betas(b).eps(eps).weight_decay(wd)) — coupled L2."""

    def __init__(self, model: BaselineUNet, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.model = model
        self.lib = model.lib
        o = _abi.AdamOpts(lr, betas[0], betas[1], eps, weight_decay)
        h = C.c_void_p()
        check(self.lib.cad_adam_create(model.h, C.byref(o), C.byref(h)), "cad_adam_create")
        self.h = h

    def step(self):
        check(self.lib.cad_adam_step(self.h, _stream(self.model.device)), "cad_adam_step")

    def zero_grad(self):
        """No-op: every backward overwrites the whole gradient slab (set_to_none semantics)."""

    def set_lr(self, lr):
        check(self.lib.cad_adam_set_lr(self.h, float(lr)), "set_lr")

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.cad_adam_destroy(h)
            self.h = None


class Optimizer:
    """The declared recipe's update rules over a U-Net's flat slab (cad_optim_*): rule "adam" (torch::optim::Adam,
    coupled L2 — the bits of `Adam` above), "adamw" (torch::optim::AdamW) or "sgd" (torch::optim::SGD with
    momentum and weight decay), trainer.h:388-414.  ema_decay > 0 keeps an exponential moving average of the
    weights in the same pass (ours; the reference has none): ema = d ema + (1 - d) p after every step, started
    as a copy of the parameters."""

    def __init__(self, model: BaselineUNet, rule="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 momentum=0.0, ema_decay=0.0):
        if not isinstance(model, BaselineUNet):   # model.h is passed on as a cad_unet*
            raise TypeError(f"cad.Optimizer serves the U-Net family (BaselineUNet and its subclasses), not "
                            f"{type(model).__name__}: the geometry-aware networks take train_step(rule=...) / optim_step, "
                            "without an EMA")
        if rule not in _abi.OPTIM_RULES:
            raise ValueError(f"rule must be one of {tuple(_abi.OPTIM_RULES)}, not {rule!r}")
        self.model, self.lib, self.rule = model, model.lib, rule
        torch.cuda.synchronize(model.device)   # the EMA starts as a copy of the parameters as they are now
        o = _abi.OptimOpts(_abi.OPTIM_RULES[rule], lr, betas[0], betas[1], eps, weight_decay, momentum, ema_decay)
        h = C.c_void_p()
        check(self.lib.cad_optim_create(model.h, C.byref(o), C.byref(h)), "cad_optim_create")
        self.h = h

    def step(self):
        check(self.lib.cad_optim_step(self.h, _stream(self.model.device)), "cad_optim_step")

    def zero_grad(self):
        """No-op: every backward overwrites the whole gradient slab (set_to_none semantics)."""

    def set_lr(self, lr):
        check(self.lib.cad_optim_set_lr(self.h, float(lr)), "set_lr")

    @property
    def lr(self) -> float:
        return float(self.lib.cad_optim_lr(self.h))

    @property
    def step_count(self) -> int:
        return int(self.lib.cad_optim_step_count(self.h))

    def state(self) -> dict:
        """Views of the device state slabs in the flat layout: m (sgd: the momentum buffer), v (None for sgd),
        ema (None without one)."""
        m, v, e = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.lib.cad_optim_state(self.h, C.byref(m), C.byref(v), C.byref(e)), "cad_optim_state")
        view = lambda p: _flat_view(p.value, self.model.n_flat, self.model.device) if p.value else None  # noqa: E731
        return {"m": view(m), "v": view(v), "ema": view(e), "step": self.step_count}

    @property
    def ema(self):
        """The averaged weights, a view of the EMA slab in the flat_params layout (None without one)."""
        return self.state()["ema"]

    def attach_ema(self, decay):
        """(Re)start the average as a copy of the current parameters."""
        check(self.lib.cad_optim_attach_ema(self.h, float(decay), _stream(self.model.device)), "attach_ema")

    def ema_swap(self):
        """Exchange the parameter and EMA slabs in place: evaluate or save the averaged model between two swaps."""
        check(self.lib.cad_optim_ema_swap(self.h, _stream(self.model.device)), "ema_swap")

    @property
    def swapped(self) -> bool:
        return bool(self.lib.cad_optim_swapped(self.h))

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.cad_optim_destroy(h)
            self.h = None


class CombinedDepthLoss:
    """CombinedDepthLoss(si_weight, grad_weight, smooth_weight, reproj_weight) with its backward
    (depth_loss.h:366-479).  forward_with_intrinsics / forward take the reference's optional
    valid_mask (bool or uint8 device tensor (B,1,H,W)); it replaces gt > 1e-6 in the SI and
    reprojection terms, the gradient-matching term ignores it (depth_loss.h:137).  height and width must be
    at least 16 (the 4-scale gradient-matching pyramid; CadError otherwise); any batch 1..batch may be passed."""

    def __init__(self, si_weight=1.0, grad_weight=0.1, smooth_weight=0.001, reproj_weight=0.01, *, batch, height,
                 width, device=0):
        self.lib = _abi.load()
        self.device = torch.device("cuda", device)
        self.weights = (si_weight, grad_weight, smooth_weight, reproj_weight)
        self.batch, self.height, self.width = batch, height, width
        self.h = self._create(reproj_weight)
        self.h_noreproj = None   # forward() (no reprojection term), created on first use

    def _create(self, reproj_weight):
        h = C.c_void_p()
        si, gr, sm, _ = self.weights
        check(self.lib.cad_loss_create(si, gr, sm, reproj_weight, self.batch, self.height, self.width,
                                       self.device.index or 0, C.byref(h)), "cad_loss_create")
        return h

    def __del__(self):
        for attr in ("h", "h_noreproj"):
            h = getattr(self, attr, None)
            if h is not None and h.value:
                self.lib.cad_loss_destroy(h)
                setattr(self, attr, None)

    def _run(self, h, pred, gt, image, intrinsics, valid_mask, loss5, dpred):
        B = pred.shape[0]
        assert pred.shape[2] == self.height and pred.shape[3] == self.width
        K = intrinsics.reshape(B, 3, 3).contiguous()
        if loss5 is None:
            loss5 = torch.empty(5, dtype=torch.float32, device=self.device)
        if dpred is None:
            dpred = torch.empty_like(pred)
        m = None
        if valid_mask is not None:
            assert valid_mask.numel() == pred.numel(), "valid_mask must be (B,1,H,W)"
            mt = valid_mask.reshape(pred.shape).to(torch.uint8).contiguous()
            m = C.c_void_p(mt.data_ptr())
        check(self.lib.cad_loss_forward_backward_masked(h, _ptr(pred), _ptr(gt), _ptr(image), _ptr(K), m, B,
                                                        _ptr(loss5), _ptr(dpred), _stream(self.device)),
              "cad_loss_forward_backward")
        return loss5, dpred

    def forward_with_intrinsics(self, pred, gt, image, intrinsics, valid_mask=None, loss5=None, dpred=None):
        """forwardWithIntrinsics + backward. Returns (loss5, dpred): loss5 = device tensor
        [total, si, grad, smooth, reproj]; dpred = dL/dpred (B,1,H,W)."""
        return self._run(self.h, pred, gt, image, intrinsics, valid_mask, loss5, dpred)

    forwardWithIntrinsics = forward_with_intrinsics

    def forward(self, pred, gt, image, valid_mask=None, loss5=None, dpred=None):
        """forward (depth_loss.h:390-404): SI + grad + smooth, no reprojection term (the kernels still
        take intrinsics for their pixel grid; identity K is passed)."""
        if self.h_noreproj is None:
            self.h_noreproj = self._create(0.0)
        B = pred.shape[0]
        K = torch.eye(3, dtype=torch.float32, device=self.device).expand(B, 3, 3).contiguous()
        return self._run(self.h_noreproj, pred, gt, image, K, valid_mask, loss5, dpred)

    def get_components_with_intrinsics(self, pred, gt, image, intrinsics, valid_mask=None):
        """getComponentsWithIntrinsics: the four terms (host floats); scratch outputs of its own, so a
        caller's loss5 / dL/dpred are left as they were."""
        loss5, _ = self.forward_with_intrinsics(pred, gt, image, intrinsics, valid_mask)
        v = loss5.cpu().tolist()
        return {"si_loss": v[1], "grad_loss": v[2], "smooth_loss": v[3], "reproj_loss": v[4]}

    getComponentsWithIntrinsics = get_components_with_intrinsics

    def get_components(self, pred, gt, image, valid_mask=None):
        loss5, _ = self.forward(pred, gt, image, valid_mask)
        v = loss5.cpu().tolist()
        return {"si_loss": v[1], "grad_loss": v[2], "smooth_loss": v[3]}

    getComponents = get_components


def depth_metrics(pred: torch.Tensor, gt: torch.Tensor) -> dict:
    """computeDepthMetrics (enhanced.h:400-439) per sample, averaged over the batch."""
    lib = _abi.load()
    B, _, H, W = pred.shape
    out = (C.c_float * 7)()
    check(lib.cad_depth_metrics(_ptr(pred), _ptr(gt), B, H, W, out, _stream(pred.device)), "cad_depth_metrics")
    keys = ["abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"]
    return {k: float(out[i]) for i, k in enumerate(keys)}


EVAL_KEYS = _abi.EVAL_KEYS   # DepthMetrics::compute's keys, in cad.h's metric order


class Evaluator:
    """Device-resident table of DepthMetrics::compute's per-sample sums (cad_evaluator, cad.h).

    update() enqueues its kernels on the current stream and returns: no allocation, no host
    synchronisation.  sums() / metrics() / summary() make one synchronous copy of the table.

    align: "none" | "median" | "log_mean" | "scale_shift" — a per-sample (scale, shift) computed on the
    device from the valid pixels (cad.h, "scale-aligned evaluation"); the metrics then score
    scale * pred + shift.  alignment() returns the (scale, shift) rows.

    depth_bins / angle_bins: ascending cuts in metres / in degrees off the optical axis (cad.h, "stratified
    evaluation"); update() then also keeps the twelve sums per sample and per stratum, strata(axis) returns
    them.  With angle_bins, update() needs the batch's K.

    geometry: also keep the surface-normal and 3-D point sums of every sample (cad.h, "geometric
    evaluation"); update() then needs the batch's K and geometry() returns them."""

    def __init__(self, capacity, max_batch, H, W, min_depth=0.1, max_depth=10.0, clamp_pred=True, device=0,
                 align="none", depth_bins=None, angle_bins=None, geometry=False):
        mode = _abi.eval_align_mode(align)
        strata = _abi.strata_config(depth_bins, angle_bins)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self._cuts = {"depth": [], "angle": []}
        self.lib = _abi.load()
        self.device = torch.device("cuda", device)
        self.capacity, self.max_batch, self.height, self.width = int(capacity), int(max_batch), int(H), int(W)
        cfg = _abi.EvalConfig(min_depth, max_depth, int(bool(clamp_pred)))
        h = C.c_void_p()
        check(self.lib.cad_evaluator_create(self.capacity, self.max_batch, self.height, self.width, C.byref(cfg), device,
                                            C.byref(h)), "cad_evaluator_create")
        self.h = h
        if mode:
            check(self.lib.cad_evaluator_set_alignment(self.h, mode), "cad_evaluator_set_alignment")
        if strata.n_depth_cuts or strata.n_angle_cuts:
            self._set_strata(strata)
        if geometry:
            self.set_geometry(True)

    def set_geometry(self, on=True):
        """Turn the geometric metrics on or off; allowed only while count == 0 (CadError otherwise)."""
        check(self.lib.cad_evaluator_set_geometry(self.h, int(bool(on))), "cad_evaluator_set_geometry")

    @property
    def geometry_on(self) -> bool:
        return bool(self.lib.cad_evaluator_get_geometry(self.h))

    def geometry(self) -> dict:
        """{"sums" (count, 8) float64 {n_normal, theta, theta^2, #<11.25, #<22.5, #<30, e, e^2}, "medians"
        (count,) float32 median theta, "metrics" (count, 9) float32 in GEOM_KEYS order, "summary"}.  CadError
        while geometry is off."""
        sums = np.zeros((self.count, _abi.GEOM_SUMS), np.float64)
        med = np.zeros((self.count,), np.float32)
        check(self.lib.cad_evaluator_geom_sums(self.h, sums.ctypes.data_as(C.POINTER(C.c_double)), _stream(self.device)),
              "cad_evaluator_geom_sums")
        check(self.lib.cad_evaluator_geom_medians(self.h, med.ctypes.data_as(_abi.FP), _stream(self.device)),
              "cad_evaluator_geom_medians")
        per, summary = eval_geom_finish(sums, med, self.sums())
        return {"sums": sums, "medians": med, "metrics": per, "summary": summary}

    def _set_strata(self, cfg):
        check(self.lib.cad_evaluator_set_strata(self.h, C.byref(cfg)), "cad_evaluator_set_strata")
        self._cuts = {"depth": [float(np.float32(c)) for c in cfg.depth_cuts[:cfg.n_depth_cuts]],
                      "angle": [float(np.float32(c)) for c in cfg.angle_cuts_deg[:cfg.n_angle_cuts]]}

    def set_strata(self, depth_bins=None, angle_bins=None):
        """Change the strata; allowed only while count == 0 (CadError otherwise, nothing changed)."""
        self._set_strata(_abi.strata_config(depth_bins, angle_bins))

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.cad_evaluator_destroy(h)
            self.h = None

    def update(self, pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor | None = None,
               K: torch.Tensor | None = None):
        """Append the B samples of pred / gt (B,1,H,W) [mask: (B,1,H,W), nonzero = valid; K: (B,3,3), the
        batch's intrinsics, required with angle_bins or geometry]."""
        B = pred.shape[0]
        assert pred.numel() == gt.numel() == B * self.height * self.width, "pred / gt must be (B,1,H,W)"
        m = None
        if mask is not None:
            assert mask.numel() == pred.numel(), "mask must be (B,1,H,W)"
            mt = mask if mask.dtype == torch.uint8 and mask.is_contiguous() else mask.to(torch.uint8).contiguous()
            m = C.c_void_p(mt.data_ptr())
        if K is None:
            check(self.lib.cad_evaluator_update(self.h, _ptr(pred), _ptr(gt), m, B, _stream(self.device)),
                  "cad_evaluator_update")
            return
        assert K.numel() == B * 9 and K.dtype == torch.float32, "K must be (B,3,3) float32"
        Kc = K.contiguous()
        check(self.lib.cad_evaluator_update_k(self.h, _ptr(pred), _ptr(gt), m, _ptr(Kc), B, _stream(self.device)),
              "cad_evaluator_update_k")

    def reset(self):
        check(self.lib.cad_evaluator_reset(self.h), "cad_evaluator_reset")

    def set_alignment(self, align):
        """Change the alignment mode; allowed only while count == 0 (CadError otherwise)."""
        check(self.lib.cad_evaluator_set_alignment(self.h, _abi.eval_align_mode(align)), "cad_evaluator_set_alignment")

    @property
    def align(self) -> str:
        mode = int(self.lib.cad_evaluator_get_alignment(self.h))
        return next(k for k, v in _abi.EVAL_ALIGN.items() if v == mode)

    def alignment(self) -> np.ndarray:
        """(count, 2) float32: the (scale, shift) of every sample; (1, 0) rows with align="none"."""
        out = np.zeros((self.count, 2), np.float32)
        check(self.lib.cad_evaluator_alignment(self.h, out.ctypes.data_as(_abi.FP), _stream(self.device)),
              "cad_evaluator_alignment")
        return out

    def aligned(self) -> np.ndarray:
        """(count,) bool: False where a fallback gave the sample's (scale, shift) (all False with "none")."""
        out = np.zeros((self.count,), np.uint8)
        check(self.lib.cad_evaluator_aligned(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8)), _stream(self.device)),
              "cad_evaluator_aligned")
        return out.astype(bool)

    @property
    def count(self) -> int:
        return int(self.lib.cad_evaluator_count(self.h))

    def sums(self) -> np.ndarray:
        """(count, 12) float64: {n, |d|/g, d^2/g, d^2, dln^2, |d|, |dlog10|, a1, a2, a3, p, g} sums."""
        out = np.zeros((self.count, 12), np.float64)
        check(self.lib.cad_evaluator_sums(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), _stream(self.device)),
              "cad_evaluator_sums")
        return out

    def strata_bins(self, axis) -> int:
        """Bins on "depth" or "angle" (cuts + 1); 0 when the axis is off."""
        return int(self.lib.cad_evaluator_strata_bins(self.h, _abi.strata_axis(axis)))

    def strata(self, axis) -> dict:
        """{"edges" (bins + 1 floats: metres, or degrees ending at 90), "sums" (count, bins, 12) float64,
        "per_sample" (count, bins, 12) float32 metrics, "summary": one dict per bin (count = the samples with
        a valid pixel in the bin)}.  CadError when the axis is off."""
        ax = _abi.strata_axis(axis)
        bins = self.strata_bins(axis)
        sums = np.zeros((self.count, max(bins, 1), 12), np.float64)
        check(self.lib.cad_evaluator_strata_sums(self.h, ax, sums.ctypes.data_as(C.POINTER(C.c_double)), _stream(self.device)),
              "cad_evaluator_strata_sums")
        per, summary = eval_strata_finish(sums)
        lo, hi = (self.min_depth, self.max_depth) if axis == "depth" else (0.0, 90.0)
        return {"edges": [lo] + list(self._cuts[axis]) + [hi], "sums": sums, "per_sample": per, "summary": summary}

    def _finish(self):
        per = np.zeros((self.count, 12), np.float32)
        s = _abi.EvalSummary()
        check(self.lib.cad_evaluator_metrics(self.h, per.ctypes.data_as(_abi.FP), C.byref(s)), "cad_evaluator_metrics")
        return per, s

    def metrics(self) -> np.ndarray:
        """(count, 12) float32 per-sample metrics in EVAL_KEYS order (a sample without a valid pixel: zeros)."""
        return self._finish()[0]

    def summary(self) -> dict:
        """{"count", "mean" | "std" | "median" | "min" | "max" | "pooled": {key: value}}."""
        s = self._finish()[1]
        out = {"count": int(s.count)}
        for stat in ("mean", "std", "median", "min", "max", "pooled"):
            out[stat] = {k: float(getattr(s, stat)[i]) for i, k in enumerate(EVAL_KEYS)}
        return out


def _summary_dict(s) -> dict:
    out = {"count": int(s.count)}
    for stat in ("mean", "std", "median", "min", "max", "pooled"):
        out[stat] = {k: float(getattr(s, stat)[i]) for i, k in enumerate(EVAL_KEYS)}
    return out


def eval_strata_finish(sums):
    """cad_eval_strata_finish (host only): (N, bins, 12) sums -> ((N, bins, 12) float32 metrics, [one summary
    dict per bin]); a bin's statistics run over the samples with a valid pixel in it."""
    sums = np.ascontiguousarray(sums, np.float64)
    if sums.ndim != 3 or sums.shape[2] != 12:
        raise ValueError("sums must be (N, bins, 12)")
    n, bins = sums.shape[0], sums.shape[1]
    per = np.zeros((n, bins, 12), np.float32)
    summ = (_abi.EvalSummary * max(bins, 1))()
    check(_abi.load().cad_eval_strata_finish(sums.ctypes.data_as(C.POINTER(C.c_double)), n, bins, per.ctypes.data_as(_abi.FP),
                                             summ), "cad_eval_strata_finish")
    return per, [_summary_dict(summ[b]) for b in range(bins)]


GEOM_KEYS = _abi.GEOM_KEYS   # cad.h's CAD_GEOM_METRICS order


def eval_geom_finish(sums, medians, total_sums):
    """cad_eval_geom_finish (host only): (N, 8) geometry sums, (N,) medians and the samples' (N, 12) total rows
    (column 0, the valid count, divides the point sums) -> ((N, 9) float32 metrics in GEOM_KEYS order, summary
    dict {"count", "count_normal", "count_point", "mean" | ... | "pooled": {key: value}}).  The normal
    statistics run over the samples with a normal-valid pixel, the point statistics over those with a valid
    pixel; the pooled median is NaN."""
    sums = np.ascontiguousarray(sums, np.float64)
    medians = np.ascontiguousarray(medians, np.float32)
    total = np.ascontiguousarray(total_sums, np.float64)
    if sums.ndim != 2 or sums.shape[1] != _abi.GEOM_SUMS:
        raise ValueError("sums must be (N, 8)")
    n = sums.shape[0]
    if medians.shape != (n,) or total.shape != (n, 12):
        raise ValueError("medians must be (N,) and total_sums (N, 12)")
    per = np.zeros((n, len(GEOM_KEYS)), np.float32)
    s = _abi.GeomSummary()
    DP = C.POINTER(C.c_double)
    check(_abi.load().cad_eval_geom_finish(sums.ctypes.data_as(DP), medians.ctypes.data_as(_abi.FP), total.ctypes.data_as(DP),
                                           n, per.ctypes.data_as(_abi.FP), C.byref(s)), "cad_eval_geom_finish")
    out = {"count": int(s.count), "count_normal": int(s.count_normal), "count_point": int(s.count_point)}
    for stat in ("mean", "std", "median", "min", "max", "pooled"):
        out[stat] = {k: float(getattr(s, stat)[i]) for i, k in enumerate(GEOM_KEYS)}
    return per, out


def depth_normals(depth, K, mask=None, min_depth=0.1, max_depth=10.0):
    """Surface normals of depth (B,1,H,W) from K (B,3,3) on the device (cad_depth_normals): (normals (B,3,H,W)
    float32, zeros where invalid; valid (B,1,H,W) bool).  A pixel is valid when it and its four neighbours
    are finite, strictly inside (min_depth, max_depth) [and mask != 0]; n faces the camera (n_z < 0)."""
    lib = _abi.load()
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    assert depth.numel() == B * H * W and depth.dtype == torch.float32, "depth must be (B,1,H,W) float32"
    assert K.numel() == B * 9 and K.dtype == torch.float32, "K must be (B,3,3) float32"
    d, Kc = depth.contiguous(), K.contiguous()
    m = None
    if mask is not None:
        assert mask.numel() == depth.numel(), "mask must be (B,1,H,W)"
        mt = mask if mask.dtype == torch.uint8 and mask.is_contiguous() else mask.to(torch.uint8).contiguous()
        m = C.c_void_p(mt.data_ptr())
    normals = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=depth.device)
    check(lib.cad_depth_normals(_ptr(d), _ptr(Kc), m, B, H, W, min_depth, max_depth, _ptr(normals), C.c_void_p(valid.data_ptr()),
                                _stream(depth.device)), "cad_depth_normals")
    return normals, valid.bool()


def strata_angle_thresholds(angle_bins) -> np.ndarray:
    """The fp32 tan^2 thresholds the evaluator compares rho^2 with, for angle cuts in degrees (host only)."""
    cuts = np.ascontiguousarray(angle_bins, np.float32)
    if cuts.ndim != 1 or cuts.size > _abi.STRATA_MAX_BINS - 1:
        raise ValueError(f"angle_bins: {cuts.size} cuts given, at most {_abi.STRATA_MAX_BINS - 1}")
    out = np.zeros_like(cuts)
    check(_abi.load().cad_strata_angle_thresholds(cuts.ctypes.data_as(_abi.FP), cuts.size, out.ctypes.data_as(_abi.FP)),
          "cad_strata_angle_thresholds")
    return out


def depth_metrics_full(pred, gt, mask=None, min_depth=0.1, max_depth=10.0, clamp_pred=True, per_sample=False,
                       align="none"):
    """DepthMetrics::compute (src/evaluation/depth_metrics.h:40-88) of a batch: the twelve metrics over
    all its valid pixels; per_sample=True: computePerSample (:93-117), a list of one dict per sample.
    align: each sample's prediction is scale-aligned first (Evaluator)."""
    _abi.eval_align_mode(align)
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    ev = Evaluator(B, B, H, W, min_depth, max_depth, clamp_pred, device=pred.device.index or 0, align=align)
    ev.update(pred, gt, mask)
    if per_sample:
        return [{k: float(v) for k, v in zip(EVAL_KEYS, row)} for row in ev.metrics()]
    return ev.summary()["pooled"]


def valid_medians(pred, gt, mask=None, min_depth=0.1, max_depth=10.0) -> torch.Tensor:
    """(B, 2) device tensor {median of pred, median of gt} over each sample's valid pixels (gt strictly
    inside (min_depth, max_depth) [and mask != 0]); exact (np.median of the float32 values), computed on
    the device by radix select.  A sample without a valid pixel gives (0, 0)."""
    lib = _abi.load()
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    assert pred.numel() == gt.numel() == B * H * W, "pred / gt must be (B,1,H,W)"
    m = None
    if mask is not None:
        assert mask.numel() == pred.numel(), "mask must be (B,1,H,W)"
        mt = mask if mask.dtype == torch.uint8 and mask.is_contiguous() else mask.to(torch.uint8).contiguous()
        m = C.c_void_p(mt.data_ptr())
    out = torch.empty((B, 2), dtype=torch.float32, device=pred.device)
    check(lib.cad_valid_medians(_ptr(pred), _ptr(gt), m, B, H, W, min_depth, max_depth, _ptr(out), _stream(pred.device)),
          "cad_valid_medians")
    return out


def _eval_forward(model, rgb, K):
    if isinstance(model, GeometryAwareNetwork):
        return model.forward(rgb, ray_directions(K, rgb.shape[2], rgb.shape[3]), camera_from_K(K))
    if getattr(model, "conditioned", False):
        return model.forward_cam(rgb, camera_from_K(K))
    return model.forward(rgb)


view = _abi.view   # cad_view of keyword fields (zoom=, zoom_x=, shift_x=, yaw=, ...); ValueError for a refused value


def _view_of(v):
    if isinstance(v, _abi.View):
        return v
    if isinstance(v, dict):
        return _abi.view(**v)
    raise ValueError(f"view must be a cad.view(...) or a dict of its fields, not {type(v).__name__}")


def _k33(K, B, what):
    if not (isinstance(K, torch.Tensor) and K.is_cuda and K.dtype == torch.float32 and tuple(K.shape) == (B, 3, 3)):
        raise ValueError(f"{what} must be a ({B},3,3) float32 device tensor")
    return K.contiguous()


def resolve_view(view, K: torch.Tensor, H: int, W: int):
    """cad_view_resolve: one view against a batch's K (B,3,3) -> (K' (B,3,3), R (B,3,3)) on the device.
    fx' = zoom_x fx, fy' = zoom_y fy, cx' = cx + shift_x W, cy' = cy + shift_y H; R = Rz(roll) Rx(pitch) Ry(yaw),
    P' = R P, the same for every sample."""
    v = _view_of(view)
    if K.dim() != 3:
        raise ValueError("K must be (B,3,3)")
    Kc = _k33(K, K.shape[0], "K")
    K_new, R = torch.empty_like(Kc), torch.empty_like(Kc)
    check(_abi.load().cad_view_resolve(C.byref(v), _ptr(Kc), Kc.shape[0], int(H), int(W), _ptr(K_new), _ptr(R),
                                       _stream(K.device)), "cad_view_resolve")
    return K_new, R


def camera_view(rgb, depth, K, view=None, K_new=None, R=None, mask=None, out=None):
    """cad_camera_view: the batch as a virtual camera records it (cad.h, "virtual cameras").  rgb (B,3,H,W),
    depth (B,1,H,W), K (B,3,3) float32 device tensors; either `view` (cad.view(...) or a dict of its fields, for
    the whole batch) or per-sample K_new and / or R (B,3,3) (missing: K / the identity); mask (B,1,H,W), non-zero
    = valid.  Returns (rgb', depth', K', valid (B,1,H,W) bool): rgb bilinear with edge replicate, depth nearest
    and divided by d.z, 0 where nothing valid is seen.  out: (rgb', depth', valid uint8) tensors to write into;
    they must not overlap the inputs."""
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.float32 and rgb.dim() == 4 and rgb.shape[1] == 3):
        raise ValueError("rgb must be a (B,3,H,W) float32 device tensor")
    B, H, W = rgb.shape[0], rgb.shape[2], rgb.shape[3]
    if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32 and tuple(depth.shape) == (B, 1, H, W)):
        raise ValueError(f"depth must be a ({B},1,{H},{W}) float32 device tensor")
    Kc = _k33(K, B, "K")
    if view is not None:
        if K_new is not None or R is not None:
            raise ValueError("give either view or K_new / R, not both")
        K_new, R = resolve_view(view, Kc, H, W)
    else:
        K_new = Kc if K_new is None else _k33(K_new, B, "K_new")
        R = torch.eye(3, dtype=torch.float32, device=rgb.device).repeat(B, 1, 1) if R is None else _k33(R, B, "R")
    m = None
    if mask is not None:
        if mask.numel() != B * H * W or not mask.is_cuda:
            raise ValueError(f"mask must be a ({B},1,{H},{W}) device tensor")
        mt = mask if mask.dtype == torch.uint8 and mask.is_contiguous() else mask.to(torch.uint8).contiguous()
        m = C.c_void_p(mt.data_ptr())
    if out is None:
        rgb_o, depth_o = torch.empty_like(rgb, memory_format=torch.contiguous_format), torch.empty_like(depth, memory_format=torch.contiguous_format)
        valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=rgb.device)
    else:
        rgb_o, depth_o, valid = out
        if not (rgb_o.shape == rgb.shape and depth_o.shape == depth.shape and valid.numel() == B * H * W and
                valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous()):
            raise ValueError("out must be (rgb', depth', valid uint8) tensors of the input shapes")
    check(_abi.load().cad_camera_view(_ptr(rgb.contiguous()), _ptr(depth.contiguous()), m, _ptr(Kc), _ptr(K_new), _ptr(R), B, H, W,
                                      _ptr(rgb_o), _ptr(depth_o), C.c_void_p(valid.data_ptr()), _stream(rgb.device)),
          "cad_camera_view")
    return rgb_o, depth_o, K_new, valid.bool()


def _set_fused_eval(model, fused_eval):
    """Apply a fused_eval= argument (None: leave the model's switch as it is); a model family without the fused
    eval forward refuses True."""
    if fused_eval is None:
        return
    if not hasattr(model, "fused_eval"):
        if fused_eval:
            raise ValueError(f"{type(model).__name__} has no fused eval forward (the U-Net families only)")
        return
    model.fused_eval(fused_eval)


def evaluate(model, batches, min_depth=0.1, max_depth=10.0, clamp_pred=True, keep_predictions=False, align="none",
             depth_bins=None, angle_bins=None, geometry=False, camera_sweep=None, view_intrinsics="true",
             fused_eval=None):
    """ModelEvaluator: eval-mode forwards over `batches` of (rgb, gt, K[, mask]) device tensors, every
    prediction scored on device (Evaluator.update) with no host synchronisation inside the loop; the
    model's train / eval mode is restored.  Returns {"keys", "per_sample" (N,12), "summary",
    "forward_ms_per_image" (events around the whole loop), "parameters", "align", "alignment" (N,2)
    (scale, shift) per sample[, "predictions" (the raw ones)]}.  depth_bins / angle_bins (Evaluator): also
    "strata": {"depth" | "angle": Evaluator.strata(axis)} for the axes asked for.  geometry=True: also
    "geometry": Evaluator.geometry(), the surface-normal and 3-D point metrics from each batch's K.
    camera_sweep ({"zoom": [0.7, 1.5], "yaw": [-7, 7]}: axis -> values, one view per value; or a list of (label,
    cad.view(...))): after the main pass over a batch every view is applied to it on the device (camera_view),
    forwarded and scored into a table of its own with the same range, clamp and align; "camera_sweep" is then a
    list of {"label", "view", "per_sample" (N,12), "summary", "alignment", "aligned", "valid_share" (the view's
    valid pixels over the main pass's)}.  view_intrinsics="true": the model is given each view's K';
    "source": the sample's own K, while the data is still the warped one (how much does the model rely on
    K?).  Strata and geometry are not computed per view; "forward_ms_per_image" stays the main pass's.
    fused_eval (None: the model's own switch): run the forwards with the fused eval forward on / off
    (BaselineUNet.fused_eval); the switch keeps the value."""
    _abi.eval_align_mode(align)
    _set_fused_eval(model, fused_eval)
    if view_intrinsics not in ("true", "source"):
        raise ValueError(f"view_intrinsics must be 'true' or 'source', not {view_intrinsics!r}")
    if camera_sweep is None:
        views = []
    elif isinstance(camera_sweep, dict):
        views = _abi.sweep_views(camera_sweep)
    else:
        views = [(str(label), _view_of(v)) for label, v in camera_sweep]
    batches = list(batches)
    if not batches:
        raise ValueError("evaluate: no batches")
    H, W = batches[0][0].shape[2], batches[0][0].shape[3]
    dev = batches[0][0].device
    n = sum(int(b[0].shape[0]) for b in batches)
    ev = Evaluator(n, max(int(b[0].shape[0]) for b in batches), H, W, min_depth, max_depth, clamp_pred,
                   device=dev.index or 0, align=align, depth_bins=depth_bins, angle_bins=angle_bins,
                   geometry=geometry)
    with_k = ev.strata_bins("angle") > 0 or ev.geometry_on
    max_b = max(int(b[0].shape[0]) for b in batches)
    view_evs = [Evaluator(n, max_b, H, W, min_depth, max_depth, clamp_pred, device=dev.index or 0, align=align)
                for _ in views]
    was_training = bool(getattr(model, "training", True))
    model.eval()
    preds = []
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spans = []   # with views: one event pair per batch around the main pass alone
    try:
        t0.record()
        for b in batches:
            rgb, gt, K = b[0], b[1], b[2]
            mask = b[3] if len(b) > 3 else None
            if views:
                spans.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                spans[-1][0].record()
            pred = _eval_forward(model, rgb, K)
            ev.update(pred, gt, mask, K if with_k else None)
            if keep_predictions:
                preds.append(pred.clone())
            if views:
                spans[-1][1].record()
            for (_, v), vev in zip(views, view_evs):
                rgb_v, gt_v, K_v, valid_v = camera_view(rgb, gt, K, view=v, mask=mask)
                # (an identity view copies the depth, masked pixels included: its valid map carries the mask on)
                vev.update(_eval_forward(model, rgb_v, K_v if view_intrinsics == "true" else K), gt_v,
                           valid_v if mask is not None else None)
        t1.record()
        per = ev.metrics()   # the first host-visible event: one copy of the table
        ms = sum(a.elapsed_time(z) for a, z in spans) if views else t0.elapsed_time(t1)
    finally:
        model.train(was_training)
    out = {"keys": EVAL_KEYS, "per_sample": per, "summary": ev.summary(), "forward_ms_per_image": ms / n,
           "parameters": model.count_parameters(), "align": align, "alignment": ev.alignment()}
    if views:
        main_valid = float(ev.sums()[:, 0].sum())
        out["view_intrinsics"] = view_intrinsics
        out["camera_sweep"] = [
            {"label": label, "view": v.as_dict(), "per_sample": vev.metrics(), "summary": vev.summary(),
             "alignment": vev.alignment(), "aligned": vev.aligned(),
             "valid_share": float(vev.sums()[:, 0].sum()) / main_valid if main_valid > 0 else 0.0}
            for (label, v), vev in zip(views, view_evs)]
    if keep_predictions:
        out["predictions"] = torch.cat(preds)
    axes = [a for a in ("depth", "angle") if ev.strata_bins(a) > 0]
    if axes:
        out["strata"] = {a: ev.strata(a) for a in axes}
    if ev.geometry_on:
        out["geometry"] = ev.geometry()
    return out


def ray_directions(K: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """RayDirectionComputer::computeRayDirections for a batch of K (B,3,3) -> (B,3,H,W)."""
    lib = _abi.load()
    B = K.shape[0]
    out = torch.empty((B, 3, height, width), dtype=torch.float32, device=K.device)
    check(lib.cad_ray_directions(_ptr(K.contiguous()), B, height, width, _ptr(out), _stream(K.device)), "rays")
    return out


class GradBucketer:
    """Decoder-first gradient buckets for the data-parallel all-reduce.

    Backward stages finish in decreasing flat-slab offset order (head, dec1..dec4, bottleneck,
    enc4..enc1), so consecutive stages form contiguous slices.  A slice is launched (async, RCCL over
    xGMI via torch.distributed) as soon as it holds >= bucket_elems floats or the last stage ends;
    the launch records an event on the current stream, so the collective overlaps the remaining
    backward kernels.  Every element is reduced exactly once (SUM; the 1/world mean is folded into
    clip + Adam)."""

    def __init__(self, flat: torch.Tensor, num_stages: int, bucket_elems: int, process_group=None):
        self.flat, self.num_stages, self.bucket_elems, self.pg = flat, num_stages, bucket_elems, process_group
        self.pending = []
        self.lo = self.hi = None
        self.buckets = []

    def on_stage(self, stage, off, cnt):
        lo, hi = off, off + cnt
        self.lo = lo if self.lo is None else min(self.lo, lo)
        self.hi = hi if self.hi is None else max(self.hi, hi)
        if self.hi - self.lo >= self.bucket_elems or stage == self.num_stages - 1:
            self.flush()

    def flush(self):
        import torch.distributed as dist
        if self.lo is None:
            return
        self.buckets.append((self.lo, self.hi))
        self.pending.append(dist.all_reduce(self.flat[self.lo:self.hi], group=self.pg, async_op=True))
        self.lo = self.hi = None

    def wait(self):
        for w in self.pending:
            w.wait()
        self.pending = []


class Communicator:
    """RCCL communicator of libcad (cad_comm_* in cad.h; C++: cad::distributed::Communicator), the
    data-parallel exchange build/train uses: one rank per GPU, rank 0's 128-byte unique id handed to
    the others out of band (a file, a torch.distributed broadcast_object_list, ...).

    backward_allreduce(model, ddepth) runs the backward with the decoder-first bucketed SUM
    all-reduce issued on the communicator's own stream as each bucket's last stage is enqueued; the
    caller's stream waits for the last one, so clip (prescale 1/world) and Adam see the reduced slab."""

    @staticmethod
    def unique_id() -> bytes:
        lib = _abi.load()
        buf = (C.c_uint8 * 128)()
        check(lib.cad_comm_get_unique_id(buf), "cad_comm_get_unique_id")
        return bytes(buf)

    def __init__(self, uid: bytes, world: int, rank: int, device: int = 0):
        assert len(uid) == 128, "unique id is 128 bytes"
        self.lib = _abi.load()
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        check(self.lib.cad_comm_create((C.c_uint8 * 128)(*uid), world, rank, device, C.byref(h)), "cad_comm_create")
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.cad_comm_destroy(h)
            self.h = None

    def rank(self) -> int:
        return self.lib.cad_comm_rank(self.h)

    def size(self) -> int:
        return self.lib.cad_comm_size(self.h)

    def set_timing(self, on=True):
        """Time every backward_allreduce from now on (cad_comm_set_timing): exposed exchange time and
        all-reduce span per call, read by stats()."""
        check(self.lib.cad_comm_set_timing(self.h, int(bool(on))), "cad_comm_set_timing")
        return self

    def stats(self) -> dict:
        """Exchange accounting since the last read (cad_comm_stats_read; waits for the recorded events):
        calls, buckets, bytes all-reduced, and over the timed calls the summed exposed time (last
        backward kernel -> compute stream released by the last all-reduce) and all-reduce span."""
        s = _abi.CommStats()
        check(self.lib.cad_comm_stats_read(self.h, C.byref(s)), "cad_comm_stats_read")
        return {"calls": s.calls, "timed_calls": s.timed_calls, "buckets": s.buckets, "bytes": s.bytes,
                "exposed_ms": s.exposed_ms, "span_ms": s.span_ms}

    def allreduce(self, t: torch.Tensor, op="sum"):
        check(self.lib.cad_comm_allreduce(self.h, _ptr(t), t.numel(), {"sum": 0, "max": 1}[op], _stream(self.device)),
              "cad_comm_allreduce")
        return t

    def broadcast_parameters(self, model, root=0):
        """Identical replicas: the flat parameter slab of `model` (any family) from rank `root`."""
        if isinstance(model, BaselineUNet):
            check(self.lib.cad_comm_broadcast_params(model.h, self.h, root, _stream(self.device)), "broadcast_params")
        else:
            check(self.lib.cad_comm_broadcast(self.h, model._flat_p, model.n_flat, root, _stream(self.device)),
                  "cad_comm_broadcast")

    def backward_allreduce(self, model, ddepth: torch.Tensor, bucket_elems=25 << 18):
        """The model's staged backward with the overlapped SUM exchange (cad_unet_backward_allreduce,
        cad_resunet_backward_allreduce, cad_geonet_backward_allreduce)."""
        fn = (self.lib.cad_unet_backward_allreduce if isinstance(model, BaselineUNet)
              else getattr(self.lib, model._PREFIX + "backward_allreduce"))
        check(fn(model.h, self.h, _ptr(ddepth), bucket_elems, _stream(self.device)), "backward_allreduce")


class Trainer:
    """One optimisation step of TensorBoardTrainerEnhanced::trainEpoch (enhanced.h:287-304):
    zero_grad, forward, forwardWithIntrinsics, backward, clip_grad_norm_(max 1.0), Adam.step.

    Data-parallel: with `process_group` set, gradient buckets are all-reduced
    (RCCL over xGMI via torch.distributed) as soon as their backward stage is enqueued, overlapping
    the rest of the backward; the mean (1/world) is folded into clip + Adam.  BN statistics and
    loss masks stay per replica (DDP semantics, no SyncBN).  With `communicator` (a libcad
    Communicator) the same exchange runs inside the library (cad_unet_backward_allreduce), as in
    build/train."""

    def __init__(self, model: BaselineUNet, loss_fn: CombinedDepthLoss, lr=1e-4, weight_decay=1e-5,
                 grad_clip=1.0, use_grad_clip=True, process_group=None, bucket_mb=25.0, communicator=None,
                 optimizer="adam", schedule=None, ema_decay=0.0, momentum=0.0, betas=(0.9, 0.999), eps=1e-8,
                 fused_eval=None):
        """fused_eval (None: leave the model's switch): the model's eval-mode forwards (validation, panels) run the
        fused eval forward; the train steps ignore it.
        optimizer / schedule / ema_decay are the declared recipe (off by default: the reference's Adam at a
        constant rate).  schedule: None, a callable step -> lr, or a dict of lr_at() keywords plus num_epochs
        and steps_per_epoch (the per-epoch schedule of build/train); it is applied before every step."""
        self.model, self.loss_fn = model, loss_fn
        _set_fused_eval(model, fused_eval)
        if optimizer == "adam" and ema_decay == 0.0 and momentum == 0.0 and tuple(betas) == (0.9, 0.999) and eps == 1e-8:
            self.optimizer = Adam(model, lr=lr, weight_decay=weight_decay)
        else:
            self.optimizer = Optimizer(model, rule=optimizer, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                       momentum=momentum, ema_decay=ema_decay)
        if isinstance(schedule, dict):
            from .recipe import lr_at
            kw = dict(schedule)
            num_epochs, spe = int(kw.pop("num_epochs")), int(kw.pop("steps_per_epoch"))
            lr_at(0, num_epochs, lr, **kw)   # an unknown scheduler fails here, not at the first step
            schedule = lambda k: lr_at(min(k // spe, num_epochs - 1), num_epochs, lr, **kw)  # noqa: E731
        self.schedule = schedule
        self.steps = 0
        self.grad_clip = grad_clip if use_grad_clip else float("inf")
        self.pg = process_group
        self.comm = communicator
        self.world = 1
        assert process_group is None or communicator is None, "one gradient exchange"
        if communicator is not None:
            self.world = communicator.size()
        if process_group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        self.pred = None
        self.loss5 = torch.zeros(5, dtype=torch.float32, device=model.device)
        self.timing = False
        self._events = []
        self._xstats = {"calls": 0, "buckets": 0, "bytes": 0}

    def set_exchange_timing(self, on=True):
        """Account the data-parallel exchange of the following steps (exchange_stats())."""
        self.timing = bool(on)
        if self.comm is not None:
            self.comm.set_timing(on)
        return self

    def exchange_stats(self) -> dict:
        """Gradient-exchange accounting since the last read: the communicator's rank count, bytes
        all-reduced, buckets, and the exposed (non-overlapped) exchange time summed over timed steps
        (libcad communicator: cad_comm_stats_read; torch.distributed: CUDA events around the wait)."""
        if self.comm is not None:
            out = self.comm.stats()
            out.update(backend="libcad RCCL communicator", comm_size=self.comm.size())
            return out
        if self.pg is None:
            return {"backend": None, "comm_size": 1, "calls": 0, "timed_calls": 0, "buckets": 0, "bytes": 0,
                    "exposed_ms": 0.0, "span_ms": None}
        import torch.distributed as dist
        torch.cuda.synchronize(self.model.device)
        out = dict(self._xstats, timed_calls=len(self._events),
                   exposed_ms=sum(a.elapsed_time(b) for a, b in self._events), span_ms=None,
                   backend=f"torch.distributed ({dist.get_backend(self.pg)})", comm_size=dist.get_world_size(self.pg))
        self._events = []
        self._xstats = {"calls": 0, "buckets": 0, "bytes": 0}
        return out

    def train_step(self, rgb, gt, K):
        m = self.model
        m.train()
        self.optimizer.zero_grad()
        B = rgb.shape[0]
        if self.pred is None or self.pred.shape[0] != B:
            self.pred = torch.empty((B, 1, m.height, m.width), dtype=torch.float32, device=m.device)
            self.dpred = torch.empty_like(self.pred)
            self.cam4 = torch.empty((B, 4), dtype=torch.float32, device=m.device)
        if m.conditioned:   # camera vector from the batch intrinsics (a15), then the FiLM forward
            check(m.lib.cad_camera_from_K(_ptr(K.reshape(B, 9).contiguous()), B, _ptr(self.cam4),
                                          _stream(m.device)), "camera_from_K")
            m.forward_cam(rgb, self.cam4, out=self.pred)
        else:
            m.forward(rgb, out=self.pred)
        self.loss_fn.forward_with_intrinsics(self.pred, gt, rgb, K, loss5=self.loss5, dpred=self.dpred)
        if self.comm is not None:
            self.comm.backward_allreduce(m, self.dpred, self.bucket_elems)
            clip_grad_norm_(m, self.grad_clip, prescale=1.0 / self.world)
        elif self.world > 1:
            bk = GradBucketer(m.flat_grads, m.num_stages, self.bucket_elems, self.pg)
            m.backward(self.dpred, on_stage=bk.on_stage)
            ev = None
            if self.timing:   # exposed exchange time: after the last backward kernel -> after the wait
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            bk.wait()
            if ev is not None:
                ev[1].record()
                self._events.append(ev)
            self._xstats["calls"] += 1
            self._xstats["buckets"] += len(bk.buckets)
            self._xstats["bytes"] += 4 * sum(hi - lo for lo, hi in bk.buckets)
            clip_grad_norm_(m, self.grad_clip, prescale=1.0 / self.world)
        else:
            m.backward(self.dpred)
            clip_grad_norm_(m, self.grad_clip)
        if self.schedule is not None:
            self.optimizer.set_lr(self.schedule(self.steps))
        self.optimizer.step()
        self.steps += 1
        return self.loss5


class ResNetUNet:
    """Config-5 network (BASELINE configs[4]): ResNet-50 encoder + U-Net decoder on MI355X, bf16
    operands (cad_resunet_*; resunet.cpp).  No reference model exists — parity is unpinned and the
    network is checked against the torch fp32 restatement in oracle/resunet_oracle.py.

    Parameter names follow torchvision's ResNet-50 under "encoder." and the U-Net decoder
    ("dec4".."dec0", "out_conv").  train_step() = forward, CombinedDepthLoss, backward,
    clip_grad_norm_, Adam (moments owned by the model)."""

    _PREFIX = "cad_resunet_"

    def _f(self, name):
        return getattr(self.lib, self._PREFIX + name)

    def __init__(self, in_channels=3, max_depth=10.0, *, batch, height, width, device=0, fp8=False):
        self.lib = _abi.load()
        self.device = torch.device("cuda", device)
        self.batch, self.height, self.width, self.max_depth = batch, height, width, max_depth
        desc = _abi.ResUnetDesc(in_channels, batch, height, width, max_depth)
        h = C.c_void_p()
        check(self._f("create")(C.byref(desc), device, C.byref(h)), "cad_resunet_create")
        self._init_handle(h)
        self.set_fp8(fp8)

    def set_fp8(self, on=True):
        """MX-fp8 forward conv-GEMMs (cad_resunet_set_fp8): every eligible forward contraction on OCP
        MXFP8 E4M3 operands (one E8M0 scale per 32 channels); the backward stays on bf16 operands."""
        check(self._f("set_fp8")(self.h, int(bool(on))), "cad_resunet_set_fp8")
        self.fp8 = bool(on)
        return self

    @property
    def fp8_units(self) -> int:
        """number of convolutions whose forward runs on MX-fp8 operands when fp8 is on"""
        return int(self._f("fp8_units")(self.h))

    def _init_handle(self, h):
        self.h = h
        self._param_info = [self._info(0, i) for i in range(self._f("num_tensors")(h, 0))]
        self._buffer_info = [self._info(1, i) for i in range(self._f("num_tensors")(h, 1))]
        p, g, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self._f("flat")(h, C.byref(p), C.byref(g), C.byref(n)), "flat")
        self.n_flat = n.value
        self._flat_p = p.value
        self._flat_g = g.value
        self.num_stages = self._f("num_stages")(h)
        self.stage_ranges = []
        for st in range(self.num_stages):
            off, cnt = C.c_int64(), C.c_int64()
            check(self._f("stage_grad_range")(h, st, C.byref(off), C.byref(cnt)), "stage range")
            self.stage_ranges.append((off.value, cnt.value))
        self.training = True

    def _info(self, kind, idx):
        name, nd, shape = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
        check(self._f("tensor_info")(self.h, kind, idx, C.byref(name), C.byref(nd), shape), "tensor_info")
        return name.value.decode(), tuple(shape[i] for i in range(nd.value))

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self._f("destroy")(h)
            self.h = None

    def train(self, mode=True):
        self.training = bool(mode)
        check(self._f("train")(self.h, int(mode)), "cad_resunet_train")
        return self

    def eval(self):
        return self.train(False)

    def count_parameters(self) -> int:
        return int(self._f("count_parameters")(self.h))

    def histograms(self, which="params") -> "OrderedDict[str, tuple]":
        """name -> (stats, counts) of every parameter ("params") or gradient ("grads") tensor: _histograms."""
        return _histograms(self, self._f("histograms"), which)

    def _get(self, kind, idx, shape):
        out = np.empty(int(np.prod(shape)) if shape else 1, np.float32)
        check(self._f("get_tensor")(self.h, kind, idx, out.ctypes.data_as(_abi.FP), out.size), "get_tensor")
        return torch.from_numpy(out.reshape(shape))

    def named_parameters(self):
        torch.cuda.synchronize(self.device)
        return OrderedDict((n, self._get(0, i, s)) for i, (n, s) in enumerate(self._param_info))

    def named_buffers(self):
        torch.cuda.synchronize(self.device)
        return OrderedDict((n, self._get(1, i, s)) for i, (n, s) in enumerate(self._buffer_info))

    def state_dict(self):
        d = self.named_parameters()
        d.update(self.named_buffers())
        return d

    def load_state_dict(self, state, strict=True):
        torch.cuda.synchronize(self.device)
        names = {n: (0, i, s) for i, (n, s) in enumerate(self._param_info)}
        names.update({n: (1, i, s) for i, (n, s) in enumerate(self._buffer_info)})
        missing = [n for n in names if n not in state]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:5]}")
        for n, (kind, i, s) in names.items():
            if n not in state:
                continue
            v = np.ascontiguousarray(torch.as_tensor(state[n]).detach().cpu().float().numpy())
            assert tuple(v.shape) == tuple(s), f"{n}: shape {v.shape} != {s}"
            check(self._f("set_tensor")(self.h, kind, i, v.ctypes.data_as(_abi.FP), v.size), f"set {n}")

    def grads(self):
        torch.cuda.synchronize(self.device)
        out = OrderedDict()
        for i, (n, s) in enumerate(self._param_info):
            g = np.empty(int(np.prod(s)), np.float32)
            check(self._f("get_grad")(self.h, i, g.ctypes.data_as(_abi.FP), g.size), "get_grad")
            out[n] = torch.from_numpy(g.reshape(s))
        return out

    def flat_grads_ptr(self) -> int:
        """Device address of the flat gradient slab (n_flat floats): the data-parallel all-reduce buffer."""
        return self._flat_g

    def debug_buffer(self, name: str) -> torch.Tensor:
        """Test hook: a buffer of the last train-mode forward as fp32 NHWC rows (cad_resunet_debug_buffer:
        "y:<conv>" stored pre-BN outputs, "scale:<bn>" / "shift:<bn>" BN-apply coefficients, "out:<block>"
        block outputs, "cat:dec<l>" a decoder's bf16 input [skip, up])."""
        n = int(self._f("debug_buffer")(self.h, name.encode(), None, 0))
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, np.float32)
        check(0 if self._f("debug_buffer")(self.h, name.encode(), out.ctypes.data_as(_abi.FP), n) == n else 1, name)
        if name.startswith(("amax", "sidx")):
            out = out.view(np.int32)
        return torch.from_numpy(out)

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        B, Cc, H, W = x.shape
        assert Cc == 3 and H == self.height and W == self.width and B <= self.batch, "input shape mismatch"
        if out is None:
            out = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        check(self._f("forward")(self.h, _ptr(x), _ptr(out), B, _stream(self.device)), "cad_resunet_forward")
        return out

    __call__ = forward

    @property
    def flat_grads(self) -> torch.Tensor:
        """A torch view of the flat gradient slab (the data-parallel all-reduce buffer)."""
        return _flat_view(self._flat_g, self.n_flat, self.device)

    @property
    def flat_params(self) -> torch.Tensor:
        return _flat_view(self._flat_p, self.n_flat, self.device)

    def backward(self, ddepth: torch.Tensor, on_stage=None):
        """Backward of the last train-mode forward; on_stage(stage, offset, count) after each stage is
        enqueued (its gradients flat_grads[offset:offset+count] are then final on the stream)."""
        st = _stream(self.device)
        if on_stage is None:
            check(self._f("backward")(self.h, _ptr(ddepth), st), self._PREFIX + "backward")
            return
        for s in range(self.num_stages):
            check(self._f("backward_stage")(self.h, s, _ptr(ddepth), st), f"backward stage {s}")
            on_stage(s, *self.stage_ranges[s])

    def _exchange_backward(self, dpred, process_group, communicator, bucket_mb):
        """backward + the data-parallel SUM exchange of the gradient slab; returns the world size."""
        if communicator is not None:
            communicator.backward_allreduce(self, dpred, int(bucket_mb * (1 << 20) / 4))
            return communicator.size()
        if process_group is not None:
            import torch.distributed as dist
            bk = GradBucketer(self.flat_grads, self.num_stages, int(bucket_mb * (1 << 20) / 4), process_group)
            self.backward(dpred, on_stage=bk.on_stage)
            acct = getattr(self, "_xacct", None)   # exchange_accounting(): events around the wait
            if acct is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            bk.wait()
            if acct is not None:
                ev[1].record()
                acct["events"].append(ev)
                acct["calls"] += 1
                acct["buckets"] += len(bk.buckets)
                acct["bytes"] += 4 * sum(hi - lo for lo, hi in bk.buckets)
                acct["pg"] = process_group
            return dist.get_world_size(process_group)
        self.backward(dpred)
        return 1

    def exchange_accounting(self, on=True):
        """torch.distributed exchange of train_step(process_group=...): count buckets / bytes and time
        the exposed wait from now on (exchange_stats()); a libcad Communicator accounts on its own
        (Communicator.set_timing / stats)."""
        self._xacct = {"events": [], "calls": 0, "buckets": 0, "bytes": 0, "pg": None} if on else None
        return self

    def exchange_stats(self) -> dict:
        import torch.distributed as dist
        a = getattr(self, "_xacct", None) or {"events": [], "calls": 0, "buckets": 0, "bytes": 0, "pg": None}
        torch.cuda.synchronize(self.device)
        out = {"calls": a["calls"], "timed_calls": len(a["events"]), "buckets": a["buckets"], "bytes": a["bytes"],
               "exposed_ms": sum(x.elapsed_time(y) for x, y in a["events"]), "span_ms": None,
               "backend": f"torch.distributed ({dist.get_backend(a['pg'])})" if a["pg"] is not None else None,
               "comm_size": dist.get_world_size(a["pg"]) if a["pg"] is not None else 1}
        if getattr(self, "_xacct", None) is not None:
            self.exchange_accounting(True)
        return out

    def clip_grad_norm_(self, max_norm: float, prescale: float = 1.0):
        check(self._f("clip_grad_norm")(self.h, float(max_norm), float(prescale), _stream(self.device)), "clip")

    def last_grad_norm(self) -> float:
        v = C.c_float()
        check(self._f("last_grad_norm")(self.h, C.byref(v), _stream(self.device)), "last_grad_norm")
        return float(v.value)

    def adam_step(self, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5):
        check(self._f("adam_step")(self.h, lr, betas[0], betas[1], eps, weight_decay, _stream(self.device)),
              "adam_step")

    def train_step(self, loss_fn: "CombinedDepthLoss", rgb, gt, K, lr=1e-4, weight_decay=1e-5, grad_clip=1.0,
                   pred=None, dpred=None, loss5=None, process_group=None, communicator=None, bucket_mb=25.0):
        """One optimisation step (enhanced.h:287-304 sequence).  Data-parallel (process_group over
        torch.distributed, or a libcad Communicator): decoder-first gradient buckets SUM-all-reduced
        while the rest of the backward runs, clipped as the mean."""
        pred = self.forward(rgb, out=pred)
        loss5, dpred = loss_fn.forward_with_intrinsics(pred, gt, rgb, K, loss5=loss5, dpred=dpred)
        world = self._exchange_backward(dpred, process_group, communicator, bucket_mb)
        self.clip_grad_norm_(grad_clip if grad_clip else float("inf"), 1.0 / world)
        self.adam_step(lr=lr, weight_decay=weight_decay)
        return loss5, pred


class GeometryAwareNetwork(ResNetUNet):
    """GeometryAwareNetworkImpl(in_channels, init_features, camera_dim, max_depth, use_pcl, use_attention)
    (src/models/geometry_aware_network.h:201-347) on MI355X (cad_geonet_*; geonet.cpp): RayEnhancedConv
    encoder with CBAM, ConvTranspose + PerspectiveCorrectionLayer + CBAM decoder, six levels.
    forward(rgb, ray_directions, camera_intrinsics (B,4)) as the reference; parameter / buffer names
    are its named_parameters() / named_buffers().  Arithmetic: the process GEMM engine (default S3,
    fp32-accurate).  train_step(): forward, CombinedDepthLoss, backward, clip_grad_norm_, Adam."""

    _PREFIX = "cad_geonet_"
    _VARIANT = 0

    def __init__(self, in_channels=3, init_features=64, camera_dim=4, max_depth=10.0, use_pcl=True,
                 use_attention=True, *, batch, height, width, device=0):
        self.lib = _abi.load()
        self.device = torch.device("cuda", device)
        self.batch, self.height, self.width, self.max_depth = batch, height, width, max_depth
        desc = _abi.GeoNetDesc(self._VARIANT, in_channels, init_features, camera_dim, max_depth, int(use_pcl),
                               int(use_attention), batch, height, width)
        h = C.c_void_p()
        check(self._f("create")(C.byref(desc), device, C.byref(h)), "cad_geonet_create")
        self._init_handle(h)

    def forward(self, rgb, ray_directions, camera_intrinsics, out=None):
        B, Cc, H, W = rgb.shape
        assert Cc == 3 and H == self.height and W == self.width and B <= self.batch, "input shape mismatch"
        assert tuple(ray_directions.shape) == (B, 3, H, W), "ray_directions must be (B, 3, H, W)"
        assert tuple(camera_intrinsics.shape) == (B, 4), "camera_intrinsics must be (B, 4) [fx, fy, cx, cy]"
        rgb, rays, cam = (t.contiguous().float() for t in (rgb, ray_directions, camera_intrinsics))
        if out is None:
            out = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        check(self._f("forward")(self.h, _ptr(rgb), _ptr(rays), _ptr(cam), _ptr(out), B, _stream(self.device)),
              "cad_geonet_forward")
        return out

    __call__ = forward

    def num_batches_tracked(self, film=False) -> int:
        return int(self._f("num_batches_tracked")(self.h, int(film)))

    def debug_buffer(self, name: str) -> torch.Tensor:
        """Test hook: a buffer of the last step as NHWC rows ("cat<l>", "dcat<l>", "x<l>", "u<l>", "z<l>",
        the pre-BN conv outputs "y1<e|d><l>", "y2<e|d><l>"; int32: the CBAM decisions "amax<e|d><l>",
        "sidx<e|d><l>")."""
        return ResNetUNet.debug_buffer(self, name)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, np.float32)
        check(0 if self._f("debug_buffer")(self.h, name.encode(), out.ctypes.data_as(_abi.FP), n) == n else 1, name)
        if name.startswith(("amax", "sidx")):
            out = out.view(np.int32)
        return torch.from_numpy(out)

    def train_step(self, loss_fn: "CombinedDepthLoss", rgb, gt, K, lr=1e-4, weight_decay=1e-5, grad_clip=1.0,
                   rays=None, pred=None, dpred=None, loss5=None, process_group=None, communicator=None,
                   bucket_mb=25.0, rule=None, momentum=0.0, betas=(0.9, 0.999), eps=1e-8):
        """One optimisation step (enhanced.h:287-304 sequence) fed the loader's batch: rays default to
        RayDirectionComputer's from K (a18), intrinsics = [K00, K11, K02, K12] (a15).  Data-parallel
        exchange as ResNetUNet.train_step.  rule: None = the reference's Adam (adam_step); "adam" / "adamw" /
        "sgd" = the declared recipe's rules (optim_step; keep to one rule per model)."""
        if rays is None:
            rays = ray_directions(K, rgb.shape[2], rgb.shape[3])
        pred = self.forward(rgb, rays, camera_from_K(K), out=pred)
        loss5, dpred = loss_fn.forward_with_intrinsics(pred, gt, rgb, K, loss5=loss5, dpred=dpred)
        world = self._exchange_backward(dpred, process_group, communicator, bucket_mb)
        self.clip_grad_norm_(grad_clip if grad_clip else float("inf"), 1.0 / world)
        if rule is None:
            self.adam_step(lr=lr, weight_decay=weight_decay)
        else:
            self.optim_step(rule, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum=momentum)
        return loss5, pred

    def optim_step(self, rule, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, momentum=0.0, ema_decay=0.0):
        """cad_geonet_optim_step: one step of "adam" / "adamw" / "sgd" on the in-handle moments (the EMA is
        U-Net-family only: ema_decay != 0 is refused)."""
        if rule not in _abi.OPTIM_RULES:
            raise ValueError(f"rule must be one of {tuple(_abi.OPTIM_RULES)}, not {rule!r}")
        o = _abi.OptimOpts(_abi.OPTIM_RULES[rule], lr, betas[0], betas[1], eps, weight_decay, momentum, ema_decay)
        check(self.lib.cad_geonet_optim_step(self.h, C.byref(o), _stream(self.device)), "cad_geonet_optim_step")


class LightweightGeometryNetwork(GeometryAwareNetwork):
    """LightweightGeometryNetworkImpl(in_channels, init_features=32, camera_dim, max_depth)
    (geometry_aware_network.h:355-440): five levels, PCL and CBAM always on."""

    _VARIANT = 1

    def __init__(self, in_channels=3, init_features=32, camera_dim=4, max_depth=10.0, *, batch, height, width,
                 device=0):
        super().__init__(in_channels, init_features, camera_dim, max_depth, True, True, batch=batch, height=height,
                         width=width, device=device)


def _flat_view(addr: int, n: int, device) -> torch.Tensor:
    """A torch view of a libcad-owned device slab (for torch.distributed collectives)."""
    class _A:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (addr, False), "version": 3}
    return torch.as_tensor(_A(), device=device)
