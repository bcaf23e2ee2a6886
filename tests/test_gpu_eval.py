"""Offline evaluation on the GPU: the fused metrics kernel (csrc/kernels/eval_kernels.hip) behind
cad_evaluator against the float64 restatement of tests/eval_restatement.py (itself checked against the
reference's fp32 arithmetic in test_eval_cpu.py), its determinism and path / batch invariance, the host
summary, consistency with the trainer's cad_depth_metrics, evaluate() over models, and build/evaluate.

Tolerance of the real-valued sums: 2e-5 relative, derived — each fp32 term carries a few ulp (division
<= 2.5 ulp, logf / log10f <= 2 ulp: ~3e-7 relative; the log difference <= 3e-7 absolute against values
of order 0.5) and the accumulation is exact to double; 2e-5 leaves ~50x headroom and is far below any
formula error.  n and the three threshold counts are exact (the inputs avoid the thresholds by 1e-4)."""
import csv
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

import eval_restatement as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
SHAPES = ((1, 5, 7), (3, 50, 70), (2, 64, 96), (2, 16, 16))


def _dev(arrs, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _sums(cad, dev, pred, gt, mask=None, lo=0.1, hi=10.0, clamp=True, splits=None):
    B, _, H, W = pred.shape
    ev = cad.Evaluator(B, B, H, W, min_depth=lo, max_depth=hi, clamp_pred=clamp)
    i = 0
    for n in splits or (B,):
        ev.update(pred[i:i + n], gt[i:i + n], None if mask is None else mask[i:i + n])
        i += n
    assert ev.count == B
    return ev.sums()


@pytest.mark.parametrize("rng_", R.RANGES)
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_match_restatement(cad, dev, shape, masked, clamp, rng_):
    """(1,5,7): scalar path, less than one block of work; (3,50,70): 16-byte path with per-sample mask
    bases that are only 4-byte aligned and more than one block per sample."""
    pred, gt, mask = R.make_inputs(*shape)
    lo, hi = rng_
    want = R.ref_sums(pred, gt, mask if masked else None, lo, hi, clamp)
    p, g, m = _dev((pred, gt, mask), dev)
    got = _sums(cad, dev, p, g, m if masked else None, lo, hi, clamp)
    with np.errstate(all="ignore"):
        print(shape, masked, clamp, rng_, np.nanmax(np.abs(got[:, R.REAL] - want[:, R.REAL]) / np.abs(want[:, R.REAL])))
    R.assert_sums_close(got, want)


def _offset(t, elems):
    """The same values in storage that starts `elems` elements past an aligned base."""
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("masked", [False, True])
def test_vector_and_scalar_paths_bit_identical(cad, dev, masked):
    pred, gt, mask = R.make_inputs(2, 64, 96)
    p, g, m = _dev((pred, gt, mask), dev)
    assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and m.data_ptr() % 4 == 0
    a = _sums(cad, dev, p, g, m if masked else None)
    po, go = _offset(p, 1), _offset(g, 1)            # one float past a 16-byte boundary: scalar path
    assert po.data_ptr() % 16 == 4 and go.data_ptr() % 16 == 4 and po.is_contiguous()
    b = _sums(cad, dev, po, go, m if masked else None)
    assert a.tobytes() == b.tobytes()
    c = _sums(cad, dev, p, _offset(g, 2), _offset(m, 1) if masked else None)   # only gt (and the mask) unaligned
    assert a.tobytes() == c.tobytes()
    R.assert_sums_close(a, R.ref_sums(pred, gt, mask if masked else None))


def test_batch_composition_invariance_and_determinism(cad, dev):
    pred, gt, mask = R.make_inputs(6, 50, 70)
    p, g, m = _dev((pred, gt, mask), dev)
    one = _sums(cad, dev, p, g, m, splits=(6,))
    two = _sums(cad, dev, p, g, m, splits=(4, 2))
    six = _sums(cad, dev, p, g, m, splits=(1,) * 6)
    assert one.tobytes() == two.tobytes() == six.tobytes()
    assert _sums(cad, dev, p, g, m, splits=(4, 2)).tobytes() == two.tobytes()
    R.assert_sums_close(one, R.ref_sums(pred, gt, mask))


def test_edge_rows(cad, dev):
    pred, gt, mask = (a.copy() for a in R.make_inputs(3, 16, 16))
    gt[1] = 0.0            # sample 1: no valid pixel
    mask[2] = 0            # sample 2: everything masked out
    p, g, m = _dev((pred, gt, mask), dev)
    ev = cad.Evaluator(4, 3, 16, 16)
    ev.update(p, g, m)
    assert ev.count == 3
    sums, per, s = ev.sums(), ev.metrics(), ev.summary()
    assert not sums[1].any() and not sums[2].any() and sums[0, 0] > 0
    assert not per[1].any() and not per[2].any()
    assert s["count"] == 3
    want = R.finish(sums)[0, 0] / 3   # the empty samples count in the mean
    assert want > 0 and abs(s["mean"]["abs_rel"] - want) <= 1e-6 * want
    R.assert_sums_close(sums, R.ref_sums(pred, gt, mask))
    # past the capacity (3 + 2 > 4) and past max_batch: an error, count and table unchanged
    with pytest.raises(cad.CadError, match="capacity"):
        ev.update(p[:2], g[:2], m[:2])
    big = torch.cat([p, p[:1]])
    with pytest.raises(cad.CadError, match="max_batch"):
        cad.Evaluator(8, 3, 16, 16).update(big, torch.cat([g, g[:1]]))
    assert ev.count == 3 and ev.sums().tobytes() == sums.tobytes()
    ev.update(p[:1], g[:1], m[:1])   # the last free row still works
    assert ev.count == 4 and ev.sums()[3].tobytes() == sums[0].tobytes()
    ev.reset()
    assert ev.count == 0 and ev.sums().shape == (0, 12) and ev.summary()["count"] == 0


def test_update_allocates_nothing(cad, dev):
    """Twenty updates between two events on a side stream leave the device's free memory as it was
    (hipMemGetInfo through torch.cuda.mem_get_info): update neither allocates nor frees.  The stream has
    carried one launch before the measurement starts (its queue exists)."""
    pred, gt, _ = R.make_inputs(2, 16, 16)
    p, g = _dev((pred, gt), dev)
    ev = cad.Evaluator(40, 2, 16, 16)
    st = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):   # the runtime builds a new stream's hardware queue at its first launch
        ev.update(p, g)
    ev.reset()
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    with torch.cuda.stream(st):
        e0.record()
        for _ in range(20):
            ev.update(p, g)
        e1.record()
    free1 = torch.cuda.mem_get_info(dev)[0]
    e1.synchronize()
    assert free0 == free1 == torch.cuda.mem_get_info(dev)[0]
    assert ev.count == 40 and e0.elapsed_time(e1) >= 0
    sums = ev.sums()
    assert all(sums[i].tobytes() == sums[i % 2].tobytes() for i in range(40))


@pytest.mark.parametrize("n", [5, 6])
def test_summary(cad, dev, n):
    pred, gt, mask = R.make_inputs(6, 16, 16)
    p, g, m = _dev((pred[:n], gt[:n], mask[:n]), dev)
    ev = cad.Evaluator(n, n, 16, 16)
    ev.update(p, g, m)
    sums = ev.sums()
    np.testing.assert_allclose(ev.metrics(), R.finish(sums), rtol=1e-6, atol=0)
    s = ev.summary()
    assert s["count"] == n
    for stat, want in R.summary(sums).items():
        got = np.array([s[stat][k] for k in R.KEYS])
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=stat)


def test_consistent_with_depth_metrics(cad, dev):
    """With the range wide open, no clamp and no mask the per-sample means equal the trainer's
    cad_depth_metrics (gt > 0; it adds 1e-8 inside the logs, which matters only below 1e-5)."""
    rng = np.random.default_rng(5)
    B, H, W = 3, 48, 64
    gt = rng.uniform(0.5, 10.0, (B, 1, H, W)).astype(np.float32)
    gt[rng.random(gt.shape) < 0.1] = 0.0
    pred = np.where(gt > 0, gt * np.exp(rng.uniform(-0.5, 0.5, gt.shape)), 1.0).astype(np.float32)
    p, g = _dev((pred, gt), dev)
    old = cad.depth_metrics(p, g)
    ev = cad.Evaluator(B, B, H, W, min_depth=1e-30, max_depth=3e38, clamp_pred=False)
    ev.update(p, g)
    new = ev.summary()["mean"]
    for k_old, k_new, tol in (("abs_rel", "abs_rel", 1e-6), ("sq_rel", "sq_rel", 1e-6), ("rmse", "rmse", 1e-6),
                              ("a1", "delta_1.25", 1e-6), ("a2", "delta_1.25^2", 1e-6), ("a3", "delta_1.25^3", 1e-6),
                              ("rmse_log", "rmse_log", 1e-5)):
        assert abs(new[k_new] - old[k_old]) <= tol * abs(old[k_old]), (k_old, new[k_new], old[k_old])


@pytest.mark.parametrize("model", ["baseline", "film"])
def test_evaluate_models(cad, dev, oracle, model):
    f, B, H, W = 4, 2, 64, 64
    cls = cad.BaselineUNet if model == "baseline" else cad.IntrinsicsConditionedUNet
    net = cls(3, f, **({} if model == "baseline" else {"camera_dim": 4}), max_depth=10.0, batch=B, height=H, width=W)
    state = dict(oracle.init_params(f, seed=3, model=model))
    state.update(oracle.init_buffers(f, model=model))
    net.load_state_dict(state)
    batches = [tuple(_dev(oracle.synth_batch(B, H, W, rgb_seed=0xC0FFEE + i, hole_seed=0xD3E7 + i), dev)) for i in range(3)]
    net.eval()
    preds = [(net.forward_cam(rgb, cad.camera_from_K(K)) if model == "film" else net.forward(rgb)).clone()
             for rgb, _, K in batches]
    net.train()
    res = cad.evaluate(net, batches)
    assert net.training, "evaluate() must restore train mode"
    allp, allg = torch.cat(preds), torch.cat([b[1] for b in batches])
    want = cad.depth_metrics_full(allp, allg, per_sample=True)
    assert res["per_sample"].shape == (6, 12) and res["summary"]["count"] == 6
    for i, row in enumerate(want):
        np.testing.assert_allclose(res["per_sample"][i], [row[k] for k in R.KEYS], rtol=1e-6, atol=0)
    pooled = cad.depth_metrics_full(allp, allg)
    np.testing.assert_allclose([res["summary"]["pooled"][k] for k in R.KEYS], [pooled[k] for k in R.KEYS], rtol=1e-6)
    assert res["parameters"] == net.count_parameters() and res["forward_ms_per_image"] > 0
    net.eval()
    cad.evaluate(net, batches[:1])
    assert not net.training, "evaluate() must restore eval mode too"


def test_cli_evaluate(cad, dev, tmp_path):
    """build/train writes a checkpoint on the synthetic dataset; build/evaluate scores it from the .pt
    and from the .cadckpt file."""
    for target in ("train", "evaluate"):
        subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", target], check=True, capture_output=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_config.yaml")))
    cfg["data"].update(num_train_samples=24, num_val_samples=8, input_height=64, input_width=96)
    cfg["training"].update(num_epochs=1, batch_size=8)
    cfg["checkpointing"]["checkpoint_dir"] = str(tmp_path / "ckpt")
    cfg["logging"]["log_dir"] = str(tmp_path / "logs")
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([os.path.join(ROOT, "build", "train"), "-c", str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ck = tmp_path / "ckpt" / "baseline_unet"
    exe = os.path.join(ROOT, "build", "evaluate")
    out = tmp_path / "eval_pt"
    r = subprocess.run([exe, "-c", str(ck / "final_model.pt"), "-g", str(p), "-o", str(out), "--save-predictions"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = list(csv.DictReader(open(out / "per_sample.csv")))
    assert len(rows) == 8 and list(rows[0]) == ["index"] + list(R.KEYS)
    summ = list(csv.DictReader(open(out / "summary.csv")))
    assert len(summ) == 1 and int(summ[0]["num_samples"]) == 8
    for k in R.KEYS:
        assert all(f"{k}_{s}" in summ[0] for s in ("mean", "std", "median", "pooled")), k
    mean = np.mean([float(x["abs_rel"]) for x in rows])
    assert abs(mean - float(summ[0]["abs_rel_mean"])) <= 1e-6 * abs(mean)
    report = (out / "report.txt").read_text()
    assert "Model Evaluation Report" in report and "AbsRel:" in report and "Median Metrics" in report
    # sample 0: the saved prediction scored in NumPy against the loader's ground truth
    pred0 = np.load(out / "pred_0.npy")
    assert pred0.shape == (64, 96) and pred0.dtype == np.float32
    seed = int(cfg.get("experiment", {}).get("seed", 42))
    ds = cad.SunRGBDDataset.synthetic(8, 64, 96, seed + 1)
    gt0 = next(iter(cad.PrefetchLoader(ds, 8, 64, 96).epoch()))[1][0].cpu().numpy()
    max_depth = float(cfg["model"].get("max_depth", 10.0))
    want = R.finish(R.ref_sums(pred0[None, None], gt0[None], None, 0.1, max_depth, True))[0]
    got = np.array([float(rows[0][k]) for k in R.KEYS])
    assert got[9] == want[9] and want[9] > 0
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=0)
    # the .cadckpt of the same weights: the identical table
    out2 = tmp_path / "eval_cadckpt"
    r = subprocess.run([exe, "-c", str(ck / "final_model.cadckpt"), "-g", str(p), "-o", str(out2)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (out2 / "per_sample.csv").read_bytes() == (out / "per_sample.csv").read_bytes()
    assert not list(out2.glob("pred_*.npy"))
