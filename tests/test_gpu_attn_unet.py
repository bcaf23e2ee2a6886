"""IntrinsicsAttentionUNet (reference src/models/intrinsics_unet.h:278-385: the FiLM U-Net with a CBAM after
every decoder block) on MI355X: the fused level-0 attention head as an operator, one training step
against the restatement (tests/attn_unet_restatement.py), the staged backward, determinism, checkpoints
and attention_maps."""
import ctypes as C
import functools
import os
import subprocess

import pytest
import torch
import yaml

from attn_unet_restatement import (AttnTrainer, attn_buffer_spec, attn_init, attn_init_buffers, attn_param_spec,
                                   level0)
from conftest import ROOT, grad_close, gpu_conv_outputs, gpu_relu_decisions, max_rel_err

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
MD = 10.0


# ---------------------------------------------------------------------------------------------
# 1, 2: the level-0 operator (cad_op_cbam_head)
# ---------------------------------------------------------------------------------------------
# (1,3,3,4): image smaller than the 7x7 window, one lane group per row; (2,5,9,16): odd sizes, a sample
# boundary inside a wave's pixel group; (3,16,24,64): the production channel count, several blocks;
# (2,8,8,128): the upper edge of head_fusable
OP_CASES = [(1, 3, 3, 4, False), (2, 5, 9, 16, False), (3, 16, 24, 64, False), (2, 8, 8, 128, False),
            (2, 5, 9, 16, True), (3, 16, 24, 64, True)]
_SHAPES = lambda C, cr: [("fc1.w", (cr, C)), ("fc1.b", (cr,)), ("fc2.w", (C, cr)), ("fc2.b", (C,)), ("sconv.w", (1, 2, 7, 7))]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _op_inputs(B, H, W, C, bf16):
    """Continuous random inputs and the fp64 autograd reference of the restated level 0, computed once
    per case and shared by the tests below (left unchanged)."""
    from oracle import cad_oracle as O
    g_ = torch.Generator().manual_seed(B * 1000 + C + (7 if bf16 else 0))
    cr = max(1, C // 16)
    y = torch.randn(B, C, H, W, generator=g_, dtype=torch.float64)
    if bf16:   # the bf16 engine's stored pre-BN outputs: both sides see the same bf16 values
        y = y.to(torch.bfloat16).double()
    scale = torch.rand(C, generator=g_, dtype=torch.float64) + 0.5
    shift = torch.rand(C, generator=g_, dtype=torch.float64) * 0.6 - 0.3
    prm = {n: (torch.rand(s, generator=g_, dtype=torch.float64) * 2 - 1) * (0.5 if n != "sconv.w" else 0.2)
           for n, s in _SHAPES(C, cr)}
    w = (torch.rand(C, generator=g_, dtype=torch.float64) * 2 - 1) / C ** 0.5
    b = torch.tensor([0.1], dtype=torch.float64)
    dpred = torch.randn(B, 1, H, W, generator=g_, dtype=torch.float64)
    p = {"a.channel_attention.fc1.weight": prm["fc1.w"], "a.channel_attention.fc1.bias": prm["fc1.b"],
         "a.channel_attention.fc2.weight": prm["fc2.w"], "a.channel_attention.fc2.bias": prm["fc2.b"],
         "a.spatial_attention.conv.weight": prm["sconv.w"]}
    leaves = list(p.values()) + [w, b, y]   # (y: so that z carries a gradient to retain)
    for v in leaves:
        v.requires_grad_(True)
    z, pred = level0(y, scale, shift, p, "a.", w, b, MD)
    z.retain_grad()
    pred.backward(dpred)
    ref = dict(pred=pred.detach().reshape(-1), z=_nhwc(z.detach()), dz=_nhwc(z.grad),
               cbam=torch.cat([v.grad.reshape(-1) for v in p.values()]), head=torch.cat([w.grad, b.grad]))
    for v in leaves:
        v.requires_grad_(False)
    packed = torch.cat([prm[n].detach().reshape(-1) for n, _ in _SHAPES(C, cr)]).float()
    return dict(y=_nhwc(y.detach()), scale=scale.float(), shift=shift.float(), packed=packed, w=w.detach().float(),
                b=b.detach().float(), dpred=dpred.reshape(-1).float(), ref=ref)


def _run_op(cad, dev, case, fused, time=False):
    B, H, W, Cc, bf16 = case
    inp = _op_inputs(*case)
    lib = cad.load_library()
    from cad_amd.model import _ptr, _stream
    y = inp["y"].to(dev).to(torch.bfloat16 if bf16 else torch.float32).contiguous()
    t = {k: inp[k].to(dev).contiguous() for k in ("scale", "shift", "packed", "w", "b", "dpred")}
    M = B * H * W
    pred = torch.empty(M, device=dev)
    dz = torch.empty(M, Cc, device=dev)
    gc, gh = torch.zeros_like(t["packed"]), torch.zeros(Cc + 1, device=dev)
    sidx = torch.empty(M, dtype=torch.int32, device=dev)
    amax = torch.empty(B * Cc, dtype=torch.int32, device=dev)
    ms = C.c_float(-1.0)
    rc = lib.cad_op_cbam_head(C.c_void_p(y.data_ptr()), int(bf16), _ptr(t["scale"]), _ptr(t["shift"]), _ptr(t["packed"]),
                              _ptr(t["w"]), _ptr(t["b"]), MD, _ptr(t["dpred"]), B, H, W, Cc, int(fused), _ptr(pred),
                              _ptr(dz), _ptr(gc), _ptr(gh), C.c_void_p(sidx.data_ptr()), C.c_void_p(amax.data_ptr()),
                              C.byref(ms) if time else None, _stream(dev))
    assert rc == 0, lib.cad_last_error()
    torch.cuda.synchronize()
    return dict(pred=pred.cpu(), dz=dz.cpu(), cbam=gc.cpu(), head=gh.cpu(), sidx=sidx.cpu(), amax=amax.cpu(), ms=ms.value)


def _op_close(got, want, mask, what):
    """max_rel_err < 1e-5 on pred, on dz where z > 0 (elsewhere the ReLU discards it) and on every CBAM and
    head gradient: the bound test_gpu_geonet.py::test_op_cbam_vs_autograd holds the generic kernels to."""
    wdz = want["dz"].reshape(got["dz"].shape)
    figs = {"pred": max_rel_err(got["pred"], want["pred"]), "dz": max_rel_err(got["dz"] * mask, wdz * mask),
            "head_w": max_rel_err(got["head"][:-1], want["head"][:-1]), "head_b": max_rel_err(got["head"][-1:], want["head"][-1:])}
    B, H, W, Cc, _ = what
    off = 0
    for n, s in _SHAPES(Cc, max(1, Cc // 16)):
        k = int(torch.tensor(s).prod())
        figs[n] = max_rel_err(got["cbam"][off: off + k], want["cbam"][off: off + k])
        off += k
    print(what, {k: "%.2e" % v for k, v in figs.items()})
    bad = {k: v for k, v in figs.items() if not v < 1e-5}
    assert not bad, (what, bad)


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "x".join(map(str, c[:4])) + ("-bf16" if c[4] else ""))
def test_op_fused_head_vs_autograd(cad, dev, case):
    """The fused level-0 attention head against fp64 autograd of the restated level 0."""
    ref = _op_inputs(*case)["ref"]
    got = _run_op(cad, dev, case, fused=1)
    _op_close(got, ref, (ref["z"] > 0).double().reshape(got["dz"].shape), case)


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "x".join(map(str, c[:4])) + ("-bf16" if c[4] else ""))
def test_op_fused_head_vs_generic(cad, dev, case):
    """... and against the generic composition (bn_relu_fwd, cbam_fwd, head_fwd, head_bwd, cbam_bwd) on the
    same inputs, at the same bound; the two argmax decisions are identical."""
    ref = _op_inputs(*case)["ref"]
    fused, generic = _run_op(cad, dev, case, fused=1), _run_op(cad, dev, case, fused=0)
    assert torch.equal(fused["sidx"], generic["sidx"]) and torch.equal(fused["amax"], generic["amax"])
    _op_close(fused, {k: v.double() for k, v in generic.items() if k != "ms"},
              (ref["z"] > 0).double().reshape(fused["dz"].shape), case)


def test_op_fused_head_refuses_other_widths(cad, dev):
    lib = cad.load_library()
    t = torch.zeros(4096, device=dev)
    from cad_amd.model import _ptr, _stream
    rc = lib.cad_op_cbam_head(_ptr(t), 0, _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), MD, _ptr(t), 1, 2, 2, 12, 1, _ptr(t),
                              _ptr(t), _ptr(t), _ptr(t), None, None, None, _stream(dev))
    assert rc != 0 and b"power of two" in lib.cad_last_error()


# ---------------------------------------------------------------------------------------------
# 3: one training step against the restatement
# ---------------------------------------------------------------------------------------------
ENGINES = {"f32": 0, "s3": 1, "bf16": 2}


@pytest.fixture
def engine(cad, request):
    lib = cad.load_library()
    prev = lib.cad_get_gemm_engine()
    assert lib.cad_set_gemm_engine(ENGINES[request.param]) == 0
    yield request.param
    lib.cad_set_gemm_engine(prev)


def _build(cad, f, B, H, W, state=None):
    net = cad.IntrinsicsAttentionUNet(3, f, 4, MD, batch=B, height=H, width=W)
    if state is not None:
        net.load_state_dict(state)
    loss = cad.CombinedDepthLoss(1.0, 0.1, 0.001, 0.01, batch=B, height=H, width=W)
    tr = cad.Trainer(net, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    return net, loss, tr


def _state(f):
    params, bufs = attn_init(f), attn_init_buffers(f)
    st = dict(params)
    st.update(bufs)
    return params, bufs, st


def _cbam_force(net):
    """The GPU run's CBAM decisions, keyed like cad_oracle.GEO_DEBUG["force"]."""
    out = {}
    for k in (1, 2, 3, 4):
        amax, sidx = net.attention_decisions(k)
        out[f"att{k}."] = (amax, sidx.reshape(-1))
    return out


def _zero_true_grad(name, B):
    # Linear bias feeding a train-mode BatchNorm1d: exactly-zero true gradient (tests/test_gpu_film.py)
    return B > 1 and (name.endswith("film.fc1.bias") or name.endswith("film.fc2.bias"))


def _ill_conditioned(name, B):
    # B == 2: FiLM's BatchNorm1d over two samples, eps-dominated gradients (tests/test_gpu_film.py)
    return B == 2 and ".film." in name and not name.endswith(("fc_gamma.bias", "fc_beta.bias"))


STEP_CASES = [(4, 2, 64, 64, "s3"), (4, 2, 64, 64, "f32"), (8, 3, 32, 48, "s3"), (8, 3, 32, 48, "bf16"),
              (16, 1, 16, 16, "s3"),    # BatchNorm1d skipped, 1x1 bottleneck
              (12, 2, 32, 32, "s3")]    # not head-fusable, no pre-split: the generic level 0


@pytest.mark.parametrize("f,B,H,W,engine", STEP_CASES, indirect=["engine"],
                         ids=[f"f{c[0]}-b{c[1]}-{c[2]}x{c[3]}-{c[4]}" for c in STEP_CASES])
def test_attn_train_step_vs_restatement(cad, dev, oracle, f, B, H, W, engine):
    """Prediction, loss, every gradient by name, the clip norm, the parameters after Adam, the BN buffers,
    the next step's prediction and the eval-mode prediction, against the restatement in fp64 next to the
    fp32 restatement's own distance from it: ours within max(floor, 3x theirs), 5x on the bf16 engine
    (whose restatement rounds the operands alike).  Floors as in tests/test_gpu_film.py: 1e-4 prediction
    and loss, grad_close(bulk_floor=5e-3), 1e-3 / 2e-3 (bf16) for the post-step predictions.  The
    restatement runs with the GPU's own ReLU and CBAM argmax decisions (exact ties at zero behind the
    ReLU); each forced CBAM choice is within 1e-4 of a true maximum.
    f=16 B=1 16x16 puts one value per channel through the bottleneck's train-mode BatchNorm2d: LibTorch's
    running_var becomes NaN there (unbiased variance of one value), and with it the reference's own
    eval-mode prediction.  Those two buffers are pinned to the engine's rule instead and the eval-mode
    comparison runs with them in the restatement; every other check of the case is the common one.

    Two fp32 witnesses (the restatement on all threads and on one: two summation orders), as
    test_gpu_geonet.py::_wider; the bounds are per tensor, max(floor, k x the further witness).

    Measured on MI355X: prediction 1.2e-7 .. 7.5e-7 from fp64 (fp32 restatement 1.3e-7 .. 1.6e-6), worst
    gradient bulk 6.5e-5 (f=4), 1.2e-3 (f=8 S3, enc4.conv.film.fc1.weight, restatement 1.4e-3), 3.2e-5
    (f=16), 5.9e-5 (f=12), 2.0e-2 (f=8 bf16, the FiLM MLPs of enc4 and dec3; restatement 1.2e-2 on both)."""
    bf16 = engine == "bf16"
    k = 5.0 if bf16 else 3.0
    ops = "bf16" if bf16 else "exact"
    params, bufs, st = _state(f)
    assert [n for n, _ in attn_param_spec(f)] == list(params)
    rgb, gt, K = [torch.from_numpy(a) for a in oracle.synth_batch(B, H, W)]
    net, loss, tr = _build(cad, f, B, H, W, st)
    assert [n for n, _ in net._param_info] == list(params)
    assert [n for n, _ in net._buffer_info] == [n for n, _ in attn_buffer_spec(f)]
    rg, gg, kg = rgb.to(dev), gt.to(dev), K.to(dev)
    cam = cad.camera_from_K(kg)
    net.train()
    pred = net.forward_cam(rg, cam)
    loss5, dpred = loss.forward_with_intrinsics(pred, gg, rg, kg)
    net.backward(dpred)
    torch.cuda.synchronize()
    grads = net.grads()
    ref = AttnTrainer(params, bufs, gemm_operands=ops)
    ref64 = AttnTrainer(params, bufs, dtype=torch.float64, gemm_operands=ops)
    oracle.GEO_DEBUG["force"] = _cbam_force(net)
    oracle.GEO_DEBUG["gap"] = []
    oracle.RELU_FORCE.update(gpu_relu_decisions(net, params, f, B, H, W, "film"))
    if bf16:
        # bf16 engine: a one-ulp fp32 difference next to a bf16 rounding boundary makes two runs' stored
        # conv outputs differ by 2^-8, far above the argmax gaps; as in the full-size bf16 tests every
        # convolution is judged on the GPU run's own stored (bf16) inputs (cad_oracle.Y_FORCE) — measured
        # without it: forced CBAM choices up to 9.8e-3 from the restatement's maxima
        oracle.Y_FORCE.update(gpu_conv_outputs(net, f, B, H, W, "film"))
    try:
        r, r64 = ref.step(rgb, gt, K), ref64.step(rgb, gt, K)
        nt = torch.get_num_threads()
        torch.set_num_threads(1)   # a second fp32 witness: another summation order (test_gpu_geonet.py::_wider)
        try:
            g32b = AttnTrainer(params, bufs, gemm_operands=ops).forward_backward(rgb, gt, K)[4]
        finally:
            torch.set_num_threads(nt)
        own = {n: max_rel_err(oracle.Y_FORCE[n], v) for n, v in oracle.Y_OWN.items()}
    finally:
        gaps = oracle.GEO_DEBUG.pop("gap", [])
        oracle.GEO_DEBUG.pop("force", None)
        oracle.RELU_FORCE.clear()
        oracle.Y_FORCE.clear()
        oracle.Y_OWN.clear()
    assert gaps and max(gaps) < 1e-4, max(gaps)
    # each convolution's own output, given the GPU's inputs, is the GPU's stored one to bf16 rounding
    assert all(v < 2.0 ** -7 for v in own.values()), max(own.items(), key=lambda kv: kv[1])
    e_pred, t_pred = max_rel_err(pred.cpu(), r64["pred"]), max_rel_err(r["pred"], r64["pred"])
    e_loss, t_loss = abs(loss5[0].item() - r64["loss"]), abs(r["loss"] - r64["loss"])
    print("pred %.2e (restatement fp32 %.2e)  loss %.2e (%.2e) of %.4f" % (e_pred, t_pred, e_loss, t_loss, r64["loss"]))
    assert e_pred < max(1e-4, k * t_pred)
    assert e_loss <= max(1e-4 * abs(r64["loss"]), k * t_loss)
    worst, bad = [], []
    # bf16 engine, the FiLM camera MLPs: the stored bf16 gradients of two fp32-accurate runs differ where a
    # value sits on a bf16 rounding boundary, by 2^-9 of that element; dgamma / dbeta sum a few dozen of them
    # at the deep levels and the BatchNorm1d over B samples amplifies the difference.  One such flip moves one
    # MLP's gradients by 1e-2, in the restatement as in our run, so a single fp32 witness can be a lucky one:
    # measured on enc4.conv.film.fc1.weight, ours 1.95e-2 from fp64, the fp32 restatement 2.0e-3 on all
    # threads and 1.2e-2 on one thread (the FiLM-only model of the same size shows the same: 7.3e-3 / 1.2e-2
    # on dec3.conv.film.fc1.weight).  Hence the two witnesses.
    for (n, _), g32, gb, g64 in zip(attn_param_spec(f), r["grads"], g32b, r64["grads"]):
        if g64 is None:   # FiLM's BatchNorm1d at batch 1: not part of the graph (no gradient, no Adam update)
            continue
        if _zero_true_grad(n, B):
            w = grads[n[: -len("bias")] + "weight"]
            assert grads[n].abs().max().item() <= 1e-2 * w.abs().max().item() + 1e-12, n
            continue
        if _ill_conditioned(n, B) or g64.abs().max().item() == 0.0:
            continue
        ok, stt = grad_close(grads[n], g64, [g32, gb], k=k, bulk_floor=5e-3)
        worst.append((stt, n))
        if not ok:
            bad.append((n, stt))
    worst.sort(reverse=True)
    print("worst gradients vs fp64 ((max, p99.9, restatement fp32 p99.9), name):", worst[:4])
    assert not bad, bad
    cad.clip_grad_norm_(net, 1.0)
    tr.optimizer.step()
    n64 = r64["norm"]
    assert abs(net.last_grad_norm() - n64) <= max(1e-4 * n64, k * abs(r["norm"] - n64)), (net.last_grad_norm(), n64)
    for n, p in net.named_parameters().items():   # Adam's first step is ~lr * sign(g)
        assert (p.double() - ref64.p[n]).abs().max().item() <= 2 * 1e-4 + 1e-6, n
    for n, b in net.named_buffers().items():
        b64 = ref64.bufs[n]
        if not torch.isfinite(b64).all():
            # B = 1 at the 1x1 bottleneck: BatchNorm2d over one value per channel.  LibTorch's running_var
            # takes the unbiased variance 0 / 0 = NaN (the restatement shows it); the engine keeps the
            # biased variance 0 for a count of 1: 0.9 * 1 + 0.1 * 0.  Nothing to compare: the engine's rule is
            # pinned, and the eval-mode forwards below run on its value
            assert B * (H >> 4) * (W >> 4) == 1 and n.startswith("bottleneck.conv.bn") and n.endswith("running_var"), n
            assert torch.equal(b, torch.full_like(b, 0.9)), n
            continue
        ours, theirs = (b.double() - b64).abs().max().item(), (ref.bufs[n].double() - b64).abs().max().item()
        assert ours <= max(1e-4 * b64.abs().max().item(), k * theirs), (n, ours, theirs)
    floor = 2e-3 if bf16 else 1e-3
    p_ref, p64 = ref.step(rgb, gt, K)["pred"], ref64.step(rgb, gt, K)["pred"]
    tr.train_step(rg, gg, kg)
    torch.cuda.synchronize()
    e, t = max_rel_err(tr.pred.cpu(), p64), max_rel_err(p_ref, p64)
    print("next-step pred %.2e (restatement fp32 %.2e)" % (e, t))
    assert e < max(floor, k * t)
    net.eval()
    pe = net.forward_cam(rg, cam)
    for n, b in net.named_buffers().items():   # (the NaN running_var of the one-value BatchNorm2d: see above)
        for t_ in (ref, ref64):
            if not torch.isfinite(t_.bufs[n]).all():
                t_.bufs[n].copy_(b)
    pe_ref, pe64 = ref.predict_eval(rgb, K), ref64.predict_eval(rgb, K)
    e, t = max_rel_err(pe.cpu(), pe64), max_rel_err(pe_ref, pe64)
    print("eval pred %.2e (restatement fp32 %.2e)" % (e, t))
    assert e < max(floor, k * t)


# ---------------------------------------------------------------------------------------------
# 4, 5: staged backward, determinism
# ---------------------------------------------------------------------------------------------
def _fwd_bwd_inputs(cad, dev, oracle, f, B, H, W):
    _, _, st = _state(f)
    rgb, gt, K = [torch.from_numpy(a).to(dev) for a in oracle.synth_batch(B, H, W)]
    net, loss, _ = _build(cad, f, B, H, W, st)
    return net, loss, st, rgb, gt, K, cad.camera_from_K(K)


@pytest.mark.parametrize("engine", ["s3", "bf16"], indirect=True)
def test_attn_staged_backward_ranges_complete(cad, dev, oracle, engine):
    """After each cad_unet_backward_stage(s) the stage's gradient range already holds what a whole
    cad_unet_backward leaves there, bit for bit (att<k> lies in stage k's range, with dec<k>)."""
    f, B, H, W = 8, 2, 32, 32
    net, loss, st, rgb, gt, K, cam = _fwd_bwd_inputs(cad, dev, oracle, f, B, H, W)
    net.train()
    pred = net.forward_cam(rgb, cam)
    _, dpred = loss.forward_with_intrinsics(pred, gt, rgb, K)
    # a sentinel no gradient takes: what a backward does not write (the alignment gaps between tensors)
    # keeps it in both runs, and a gradient a stage has not written yet shows as the sentinel
    sentinel = 12345.0
    net.flat_grads.fill_(sentinel)
    net.backward(dpred)
    torch.cuda.synchronize()
    whole = net.flat_grads.clone()
    assert (whole != sentinel).sum().item() == net.count_parameters() + 5 * f * 9   # (+ enc1.conv1's zero input channels)
    net.load_state_dict(st)
    net.forward_cam(rgb, cam)
    net.flat_grads.fill_(sentinel)
    seen = []

    def on_stage(s, off, cnt):
        torch.cuda.synchronize()
        seen.append(s)
        assert torch.equal(net.flat_grads[off: off + cnt], whole[off: off + cnt]), s
    net.backward(dpred, on_stage=on_stage)
    assert seen == list(range(10))
    names = [n for n, _ in net._param_info]
    g = net.grads()
    assert all(torch.isfinite(g[n]).all() for n in names)


def test_attn_step_is_deterministic(cad, dev, oracle):
    """Two identical steps give bit-identical predictions and gradients (no atomics on the path)."""
    f, B, H, W = 8, 3, 32, 48
    net, loss, st, rgb, gt, K, cam = _fwd_bwd_inputs(cad, dev, oracle, f, B, H, W)
    net.train()
    runs = []
    for _ in range(2):
        net.load_state_dict(st)
        pred = net.forward_cam(rgb, cam)
        _, dpred = loss.forward_with_intrinsics(pred, gt, rgb, K)
        net.backward(dpred)
        torch.cuda.synchronize()
        runs.append((pred.clone(), net.flat_grads.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1].abs().max().item() > 0


# ---------------------------------------------------------------------------------------------
# 6: checkpoints
# ---------------------------------------------------------------------------------------------
def test_attn_torch_archive_roundtrip(cad, dev, oracle, tmp_path):
    """save_torch: PyTorch reads the archive with exactly attn_param_spec's names plus the buffers, in
    order, and the constructors' module tree (the parameterless avg_pool / max_pool included); load_torch
    into a fresh model predicts identically; a checkpoint of the other FiLM model is refused by name."""
    f, B, H, W = 8, 2, 32, 32
    net, loss, st, rgb, gt, K, cam = _fwd_bwd_inputs(cad, dev, oracle, f, B, H, W)
    tr = cad.Trainer(net, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    tr.train_step(rgb, gt, K)   # running statistics and counters off their defaults
    path = tmp_path / "attn.pt"
    cad.save(net, path)
    m = torch.jit.load(str(path))
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in attn_param_spec(f)]
    assert [n for n, _ in m.named_buffers() if not n.endswith("num_batches_tracked")] == [n for n, _ in attn_buffer_spec(f)]
    sd = m.state_dict()
    nbt = [n for n in sd if n.endswith("num_batches_tracked")]
    assert len(sd) == len(attn_param_spec(f)) + len(attn_buffer_spec(f)) + len(nbt) and len(nbt) == len(attn_buffer_spec(f)) // 2
    mods = [n for n, _ in m.named_modules()]
    i = mods.index("att4.channel_attention")
    assert mods[i: i + 5] == ["att4.channel_attention"] + ["att4.channel_attention." + s for s in ("avg_pool", "max_pool", "fc1", "fc2")]
    assert mods.index("dec1") < mods.index("att4") < mods.index("att1") < mods.index("out_conv")
    for n, v in net.named_parameters().items():
        assert torch.equal(sd[n], v), n
    fresh = cad.IntrinsicsAttentionUNet(3, f, 4, MD, batch=B, height=H, width=W)
    cad.load(fresh, path)
    net.eval()
    fresh.eval()
    assert torch.equal(fresh.forward_cam(rgb, cam), net.forward_cam(rgb, cam))
    assert fresh.num_batches_tracked() == net.num_batches_tracked() == 1
    # the other model of the pair, either way round: both counts and the architecture value to use
    film = cad.IntrinsicsConditionedUNet(3, f, 4, MD, batch=B, height=H, width=W)
    n_attn, n_film = net.count_parameters(), film.count_parameters()
    with pytest.raises(cad.CadError) as e:
        cad.load(film, path)
    assert all(s in str(e.value) for s in (str(n_attn), str(n_film), "model.architecture: intrinsics_attention_unet"))
    fpath = tmp_path / "film.pt"
    cad.save(film, fpath)
    with pytest.raises(cad.CadError) as e:
        cad.load(fresh, fpath)
    assert all(s in str(e.value) for s in (str(n_attn), str(n_film), "model.architecture: intrinsics_unet"))


def test_cli_attn_train_resume_bit_for_bit(tmp_path):
    """build/train on model.architecture: intrinsics_attention_unet: two epochs in one run, and the second
    epoch again from the first epoch's .cadckpt (parameters, BN buffers, Adam state): the resumed step
    reproduces the uninterrupted one bit for bit.  An intrinsics_unet checkpoint is refused."""
    for target in ("train",):
        subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", target], check=True, capture_output=True)
    train = os.path.join(ROOT, "build", "train")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_config.yaml")))
    cfg["data"].update(dataset_name="synthetic", num_train_samples=4, num_val_samples=2, input_height=32, input_width=48)
    cfg["model"].update(architecture="intrinsics_attention_unet", init_features=8)
    cfg["training"].update(num_epochs=2, batch_size=4, val_interval=1)

    def run(tag, resume=None, arch=None, epochs=2):
        cfg["checkpointing"].update(checkpoint_dir=str(tmp_path / tag / "ckpt"), save_interval=1)
        cfg["logging"]["log_dir"] = str(tmp_path / tag / "logs")
        cfg["training"]["num_epochs"] = epochs
        if arch:
            cfg["model"]["architecture"] = arch
        p = tmp_path / (tag + ".yaml")
        p.write_text(yaml.safe_dump(cfg))
        cmd = [train, "-c", str(p)] + (["-r", str(resume)] if resume else [])
        return subprocess.run(cmd, capture_output=True, text=True, timeout=300), tmp_path / tag / "ckpt" / "baseline_unet"
    r, a = run("a")
    assert r.returncode == 0, r.stderr
    assert "Model: intrinsics_attention_unet" in r.stdout
    r, b = run("b", resume=a / "baseline_unet_epoch_1.cadckpt")
    assert r.returncode == 0 and "optimizer step 1" in r.stdout, r.stderr
    assert (a / "baseline_unet_epoch_2.cadckpt").read_bytes() == (b / "baseline_unet_epoch_2.cadckpt").read_bytes()
    r, _ = run("c", resume=a / "final_model.cadckpt", arch="intrinsics_unet", epochs=3)
    assert r.returncode == 1 and "set model.architecture: intrinsics_attention_unet" in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------
# 7: attention maps
# ---------------------------------------------------------------------------------------------
def test_attention_maps_vs_restatement(cad, dev, oracle):
    """attention_maps(level) = CBAMImpl::getAttentionMaps of att<level> for the last forward: the channel
    attention [B, C] and the spatial attention [B, 1, H_l, W_l], within 1e-5 of the restatement's."""
    from oracle import cad_oracle as O
    import torch.nn.functional as F
    f, B, H, W = 8, 2, 32, 48
    params, bufs, st = _state(f)
    rgb, gt, K = [torch.from_numpy(a) for a in oracle.synth_batch(B, H, W)]
    net, _, _ = _build(cad, f, B, H, W, st)
    net.eval()
    net.forward_cam(rgb.to(dev), cad.camera_from_K(K.to(dev)))
    torch.cuda.synchronize()
    keep = {}
    t64 = AttnTrainer(params, bufs, dtype=torch.float64)
    t64.predict_eval(rgb, K, keep)
    for k in (1, 2, 3, 4):
        pre, z = f"att{k}.", keep[f"z{k}"]
        Bc, Cc = z.shape[:2]
        mlp = lambda v: F.linear(F.relu(F.linear(v, t64.p[pre + "channel_attention.fc1.weight"], t64.p[pre + "channel_attention.fc1.bias"])),
                                 t64.p[pre + "channel_attention.fc2.weight"], t64.p[pre + "channel_attention.fc2.bias"])
        att = torch.sigmoid(mlp(F.adaptive_avg_pool2d(z, 1).view(Bc, Cc)) + mlp(F.adaptive_max_pool2d(z, 1).view(Bc, Cc)))
        x1 = z * att.view(Bc, Cc, 1, 1)
        s = torch.cat([x1.mean(1, keepdim=True), x1.max(1, keepdim=True)[0]], 1)
        sa = torch.sigmoid(F.conv2d(s, t64.p[pre + "spatial_attention.conv.weight"], None, 1, 3))
        # (the pieces above are cad_oracle._cbam's own: their product must be its output)
        assert torch.allclose(x1 * sa, O._cbam(z, t64.p, pre), rtol=0, atol=1e-12)
        ca, sp = net.attention_maps(k)
        assert tuple(ca.shape) == (B, f << (k - 1)) and tuple(sp.shape) == (B, 1, H >> (k - 1), W >> (k - 1))
        assert max_rel_err(ca, att) < 1e-5 and max_rel_err(sp, sa) < 1e-5, (k, max_rel_err(ca, att), max_rel_err(sp, sa))
    with pytest.raises(ValueError):
        net.attention_maps(5)
