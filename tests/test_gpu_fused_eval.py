"""Fused eval forward (DESIGN.md §3 "Fused eval forward"; csrc/kernels/epilogues.hpp EpiStoreAct): in eval mode the
BatchNorm affine, the ReLU and the FiLM modulation of a DoubleConv are applied to the convolution's accumulator in
the GEMM epilogue, so the pre-BN output is never written and the second pass over it is gone.

  operators  cad_op_conv3x3_fwd_act / _act_bf16 against the fp64 expression, on every window block shape and on the
             im2col kernels, with per-sample FiLM constants and an output view inside a wider row;
  models     S3 engine: prediction and every activation both paths write are bit-identical to the two-pass
             forward (the same fp32 expression on the same fp32 accumulator); bf16 engine: the activation is
             rounded once instead of twice, so it is held to the bf16-operand fp64 oracle at the bound
             tests/test_gpu_model.py holds the bf16 engine's prediction to, next to the two-pass forward;
  train mode ignores the switch; build/evaluate --fused-forward writes byte-identical tables.
"""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F
import yaml

from attn_unet_restatement import attn_init, attn_init_buffers
from conftest import ROOT, max_rel_err
from test_gpu_ops import B1_WIN_SHAPES, TOL
from test_gpu_s3_wtwin import FWD_SHAPES

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
IM2COL = (3, 5, 16, 8, 64)   # one 256-row tile holds rows of three samples (80 each) and tail rows past M = 240
CONFIGS = ("bn", "film", "view")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture
def engine(cad):
    lib = cad.load_library()
    prev = lib.cad_get_gemm_engine()

    def use(e):
        assert lib.cad_set_gemm_engine(e) == 0
        return lib
    yield use
    lib.cad_set_gemm_engine(prev)


_REF = {}


def _case(shape, bf16_operands):
    """Inputs and the fp64 references of one shape, computed once: x NHWC, w OHWI, scale in +-[0.5, 1.5] (both
    signs), shift ~ N(0, 0.3), gamma / beta different per sample; ref["bn"] = max(conv * scale + shift, 0),
    ref["film"] = gamma[b] * ref["bn"] + beta[b], NHWC fp64."""
    key = (shape, bf16_operands)
    if key not in _REF:
        B, H, W, cin, cout = shape
        g = torch.Generator().manual_seed(31 * B + 7 * H + W + cin + 3 * cout)
        x = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
        if bf16_operands:   # the twin the engine reads, and the weights as the engine rounds them
            x = x.bfloat16().float()
        wq = w.bfloat16().float() if bf16_operands else w
        sign = torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0)
        scale = sign * (0.5 + torch.rand(cout, generator=g))
        shift = 0.3 * torch.randn(cout, generator=g)
        gam = 0.5 + torch.rand(B, cout, generator=g)
        bet = 0.2 * torch.randn(B, cout, generator=g)
        y = F.conv2d(x.double(), wq.double(), None, 1, 1).permute(0, 2, 3, 1)   # NHWC
        z = y * scale.double() + shift.double()
        clipped = (z <= 0).double().mean().item()
        assert 0.2 < clipped < 0.8, clipped   # the ReLU bites on both sides
        bn = z.clamp_min(0)
        film = gam.double()[:, None, None, :] * bn + bet.double()[:, None, None, :]
        _REF[key] = dict(x=x.permute(0, 2, 3, 1).contiguous(), w=w.permute(0, 2, 3, 1).contiguous(), scale=scale,
                         shift=shift, gam=gam, bet=bet, bn=bn, film=film)
    return _REF[key]


def _run_op(lib, dev, shape, cfg, bf16_engine, out_bf16):
    """One fused convolution into a buffer pre-filled with 7: (the view's values as fp32 on the host, the reference,
    whether everything outside the view still holds 7)."""
    B, H, W, cin, cout = shape
    c = _case(shape, bf16_engine)
    film = cfg != "bn"
    ld, off = (cout + 24, 8) if cfg == "view" else (cout, 0)
    dt = torch.bfloat16 if out_bf16 else torch.float32
    ybuf = torch.full((B, H, W, ld), 7.0, dtype=dt, device=dev)
    xg = c["x"].to(dev).to(torch.bfloat16 if bf16_engine else torch.float32).contiguous()
    t = {k: c[k].to(dev).contiguous() for k in ("w", "scale", "shift", "gam", "bet")}
    fn = lib.cad_op_conv3x3_fwd_act_bf16 if bf16_engine else lib.cad_op_conv3x3_fwd_act
    rc = fn(_p(xg), cin, 0, cin, _p(t["w"]), cout, _p(t["scale"]), _p(t["shift"]), _p(t["gam"]) if film else None,
            _p(t["bet"]) if film else None, _p(ybuf), ld, off, int(out_bf16), B, H, W, _s())
    assert rc == 0, lib.cad_last_error()
    torch.cuda.synchronize()
    out = ybuf.float().cpu()
    outside = torch.cat([out[..., :off].flatten(), out[..., off + cout:].flatten()])
    return out[..., off:off + cout], c["film" if film else "bn"], bool((outside == 7.0).all())


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shape", FWD_SHAPES + [IM2COL], ids=lambda s: "x".join(map(str, s)))
def test_op_s3_vs_fp64(engine, dev, shape, cfg):
    """S3 engine: every window block shape (k_conv3x3_win_s3, with the weight twin as the default build runs it)
    and the im2col kernel enc1.conv1 takes, within test_gpu_ops.py's 2e-5 of the fp64 expression."""
    lib = engine(1)
    got, ref, untouched = _run_op(lib, dev, shape, cfg, False, False)
    err = max_rel_err(got, ref)
    print(shape, cfg, "max rel err", err)
    assert err < TOL, err
    assert untouched, "stored outside the output view"


def test_op_f32_engine_shares_the_epilogue(engine, dev):
    """CAD_GEMM_F32 runs the same epilogue on the f32 im2col kernel (gemm_epilogue_t), tall and square tiles."""
    lib = engine(0)
    for shape in (IM2COL, FWD_SHAPES[2]):
        for cfg in CONFIGS:
            got, ref, untouched = _run_op(lib, dev, shape, cfg, False, False)
            assert max_rel_err(got, ref) < TOL and untouched, (shape, cfg)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shape", B1_WIN_SHAPES + [IM2COL], ids=lambda s: "x".join(map(str, s)))
def test_op_bf16_engine_vs_fp64(engine, dev, shape, cfg):
    """bf16 engine on the pre-split twins (B1 window kernels of every tile shape, and the pre-split im2col kernel)
    against the fp64 contraction of the bf16-rounded operands: fp32 output within 2e-5; bf16 output within 2e-5
    plus half a bf16 ulp of the reference value (2^-9 |ref|) per element."""
    lib = engine(2)
    got, ref, untouched = _run_op(lib, dev, shape, cfg, True, False)
    err = max_rel_err(got, ref)
    print(shape, cfg, "fp32 out max rel err", err)
    assert err < TOL, err
    assert untouched
    got, ref, untouched = _run_op(lib, dev, shape, cfg, True, True)
    # half a bf16 ulp of the reference value: bf16 keeps 8 significant bits, so ulp(v) = 2^(floor(log2 |v|) - 7) and
    # round-to-nearest moves v by at most 2^(floor(log2 |v|) - 8) — between 2^-9 |v| (just below a power of two)
    # and 2^-8 |v| (just above one; the exactly rounded reference itself sits there)
    half_ulp = torch.where(ref == 0, torch.zeros_like(ref), torch.exp2(torch.floor(torch.log2(ref.abs())) - 8))
    excess = ((got.double() - ref).abs() - half_ulp).max().item() / ref.abs().max().item()
    print(shape, cfg, "bf16 out excess over half an ulp", excess)
    assert excess < TOL, excess
    assert untouched


# ---------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------
FM, BM, HM, WM = 64, 2, 16, 128   # level widths 128 .. 8: all five window shapes at f = 64, im2col enc1.conv1
KINDS = {"baseline": "BaselineUNet", "film": "IntrinsicsConditionedUNet", "rayfilm": "RayConditionedUNet",
         "attn": "IntrinsicsAttentionUNet"}


def _state(oracle, kind, f):
    """init_params (the attention family: its own initialiser) with every BatchNorm weight / bias, every running
    mean / variance and the FiLM output layers overwritten by seeded random values: the initial buffers
    (mean 0, variance 1) would let a dropped shift pass."""
    if kind == "attn":
        params, bufs = attn_init(f), attn_init_buffers(f)
    else:
        params, bufs = oracle.init_params(f, seed=11, model=kind), oracle.init_buffers(f, model=kind)
    g = torch.Generator().manual_seed(77)
    params = {k: v.clone() for k, v in params.items()}
    bufs = {k: v.clone() for k, v in bufs.items()}
    for n, v in params.items():
        if ".bn" in n:
            params[n] = (0.5 + torch.rand(v.shape, generator=g)) if n.endswith("weight") else 0.2 * torch.randn(v.shape, generator=g)
        elif ".fc_gamma." in n or ".fc_beta." in n:
            if n.endswith("weight"):
                params[n] = 0.1 * torch.randn(v.shape, generator=g)
            elif ".fc_gamma." in n:
                params[n] = 0.5 + torch.rand(v.shape, generator=g)
            else:
                params[n] = 0.2 * torch.randn(v.shape, generator=g)
    for n, v in bufs.items():
        bufs[n] = 0.3 * torch.randn(v.shape, generator=g) if n.endswith("mean") else 0.5 + 1.5 * torch.rand(v.shape, generator=g)
    state = dict(params)
    state.update(bufs)
    return params, bufs, state


def _inputs(oracle, B, H, W, dev):
    rgb, gt, K = [torch.from_numpy(a) for a in oracle.synth_batch(B, H, W)]
    K = K.clone()
    K[1, 0, 0] *= 1.3   # two different cameras in the batch
    K[1, 1, 1] *= 0.8
    K[1, 0, 2] += 9.0
    return rgb, gt, K


def _forward(cad, m, rgb, K):
    if m.conditioned:
        return m.forward_cam(rgb, cad.camera_from_K(K))
    return m.forward(rgb)


def _activations(m):
    names = [f"enc{l}_a1" for l in range(5)] + [f"dec{l}_a1" for l in range(4)] + [f"cat{l}" for l in range(4)] + \
            ["bott"] + [f"pool{l}" for l in range(1, 5)] + [f"dout{l}" for l in range(1, 4)]
    return {n: m.debug_buffer(n).clone() for n in names}


@pytest.mark.parametrize("kind", list(KINDS))
def test_model_s3_bit_identical(cad, engine, dev, oracle, kind):
    engine(1)
    _, _, state = _state(oracle, kind, FM)
    rgb, _, K = _inputs(oracle, BM, HM, WM, dev)
    rgb, K = rgb.to(dev), K.to(dev)
    args = (3, FM, 10.0) if kind == "baseline" else (3, FM, 4, 10.0)
    m = getattr(cad, KINDS[kind])(*args, batch=BM, height=HM, width=WM)
    m.load_state_dict(state)
    m.eval()
    assert not m.fused_eval_on()
    for B in (BM, 1):   # the full batch, then a partial one on the same handle
        m.fused_eval(False)
        p0 = _forward(cad, m, rgb[:B].contiguous(), K[:B].contiguous()).clone()
        torch.cuda.synchronize()
        assert m.fused_eval_convs() == (0, 18)
        a0 = _activations(m)
        m.fused_eval(True)
        p1 = _forward(cad, m, rgb[:B].contiguous(), K[:B].contiguous()).clone()
        torch.cuda.synchronize()
        # every 3 x 3 convolution but dec1.conv2, whose y2 the fused level-0 head (attention head) reads
        assert m.fused_eval_convs() == (17, 18)
        a1 = _activations(m)
        assert torch.isfinite(p0).all() and p0.std().item() > 1e-3
        if B > 1 and kind != "baseline":
            assert not torch.equal(p0[0], p0[1])
        for n in a0:
            d = (a0[n] - a1[n]).abs().max().item()
            assert torch.equal(a0[n], a1[n]), (kind, B, n, d)
        assert torch.equal(p0, p1), (kind, B, (p0 - p1).abs().max().item())


@pytest.mark.parametrize("kind", ["baseline", "rayfilm"])
def test_train_mode_ignores_the_switch(cad, engine, dev, oracle, kind):
    engine(1)
    _, _, state = _state(oracle, kind, FM)
    rgb, gt, K = [t.to(dev) for t in _inputs(oracle, BM, HM, WM, dev)]
    runs = []
    for on in (False, True):
        args = (3, FM, 10.0) if kind == "baseline" else (3, FM, 4, 10.0)
        m = getattr(cad, KINDS[kind])(*args, batch=BM, height=HM, width=WM)
        m.load_state_dict(state)
        loss = cad.CombinedDepthLoss(1.0, 0.1, 0.001, 0.01, batch=BM, height=HM, width=WM)
        tr = cad.Trainer(m, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0, fused_eval=on)
        assert m.fused_eval_on() == on
        losses, norms = [], []
        for _ in range(3):
            losses.append(tr.train_step(rgb, gt, K).clone())
            norms.append(m.last_grad_norm())
            assert m.fused_eval_convs() == (0, 18)
        torch.cuda.synchronize()
        m.eval()
        pe = _forward(cad, m, rgb, K).clone()
        torch.cuda.synchronize()
        assert m.fused_eval_convs()[0] == (17 if on else 0)
        runs.append((torch.stack(losses), norms, m.flat_params.clone(), pe))
    off, on = runs
    assert torch.isfinite(off[0]).all() and off[1][0] > 0
    assert torch.equal(on[0], off[0]), "losses differ"
    assert on[1] == off[1], "gradient norms differ"
    assert torch.equal(on[2], off[2]), "parameters differ"
    assert torch.equal(on[3], off[3]), "eval forward after the steps differs"


@pytest.mark.parametrize("kind", ["baseline", "rayfilm"])
def test_model_bf16_engine_vs_oracle(cad, engine, dev, oracle, kind):
    """48 x 128 at f = 64 (test_gpu_model.py's shape that covers every B1 window block).  Yardstick: the oracle
    with bf16-rounded operands in fp64; bound: test_gpu_model.py's for a prediction on this engine,
    max(1e-3, 5 x the fp32 run of the same arithmetic's own distance from fp64).  The two-pass forward must meet
    it too (the yardstick itself)."""
    engine(2)
    f, B, H, W = 64, 2, 48, 128
    params, bufs, state = _state(oracle, kind, f)
    rgb, _, K = _inputs(oracle, B, H, W, dev)
    ref32 = oracle.Trainer(params, bufs, model=kind, gemm_operands="bf16")
    ref64 = oracle.Trainer(params, bufs, model=kind, dtype=torch.float64, gemm_operands="bf16")
    Kin = None if kind == "baseline" else K
    pe32, pe64 = ref32.predict_eval(rgb, Kin), ref64.predict_eval(rgb, Kin)
    bound = max(1e-3, 5 * max_rel_err(pe32, pe64))
    args = (3, f, 10.0) if kind == "baseline" else (3, f, 4, 10.0)
    m = getattr(cad, KINDS[kind])(*args, batch=B, height=H, width=W)
    m.load_state_dict(state)
    m.eval()
    errs = {}
    for on in (False, True):
        m.fused_eval(on)
        p = _forward(cad, m, rgb.to(dev), K.to(dev)).cpu()
        assert m.fused_eval_convs() == ((17, 18) if on else (0, 18))
        errs[on] = max_rel_err(p, pe64)
    print(kind, "bf16 engine vs bf16-operand fp64 oracle: two-pass", errs[False], "fused", errs[True], "bound", bound)
    assert errs[False] < bound, ("two-pass", errs[False], bound)
    assert errs[True] < bound, ("fused", errs[True], bound)


def test_cli_evaluate_fused_forward(cad, dev, tmp_path):
    """build/evaluate on the synthetic dataset with and without --fused-forward (default engine): the tables are
    byte-identical and stdout names the mode."""
    subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", "evaluate"], check=True, capture_output=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_config.yaml")))
    cfg["data"].update(num_train_samples=8, num_val_samples=6, input_height=32, input_width=64)
    cfg["training"].update(batch_size=4)
    cfg["model"].update(architecture="baseline_unet", init_features=16)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    m = cad.BaselineUNet(3, 16, float(cfg["model"].get("max_depth", 10.0)), batch=4, height=32, width=64)
    ck = tmp_path / "model.pt"
    cad.save(m, str(ck))
    exe = os.path.join(ROOT, "build", "evaluate")
    outs = {}
    for flag in ((), ("--fused-forward",)):
        out = tmp_path / ("fused" if flag else "plain")
        r = subprocess.run([exe, "-c", str(ck), "-g", str(p), "-o", str(out), *flag], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        outs[bool(flag)] = (out, r.stdout)
    assert "Forward mode: two-pass eval forward, fused 0 of 18 convolutions" in outs[False][1]
    assert "Forward mode: fused eval forward, fused 17 of 18 convolutions" in outs[True][1]
    for name in ("per_sample.csv", "summary.csv"):
        a, b = (outs[False][0] / name).read_bytes(), (outs[True][0] / name).read_bytes()
        assert len(a) > 0 and a == b, name
