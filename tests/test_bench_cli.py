"""bench.py's command line: a plain run measures the headline only, --full adds the other legs, and
--dump-outputs DIR writes what the last timed step handed its caller.

  * CPU: the defaults (--full off, no dump), the fixed sample of an output too large to store whole,
    and the 64 MB bound of a dump at any shape;
  * GPU: one plain run at a tiny shape in a process of its own: the JSON line carries the headline
    fields and none of the --full legs, --steps sets the timed steps, and the dumped arrays equal what
    the same warm-up + timed steps give in this process from the same fixed inputs and initial weights
    (the U-Net step is deterministic: DESIGN.md §3)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

TINY = dict(batch=2, height=64, width=64, features=8, steps=3, warmup=1)


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_plain_run_is_the_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_sample_fixed_and_bounded():
    bench = _bench()
    x = np.arange(1000, dtype=np.float64) * 0.5
    whole = bench.dump_sample(x.reshape(10, 100), 1000)
    assert whole.dtype == np.float32 and whole.shape == (10, 100) and np.array_equal(whole, x.reshape(10, 100))
    s1, s2 = bench.dump_sample(x, 64), bench.dump_sample(x.copy(), 64)
    assert s1.dtype == np.float32 and s1.shape == (64,) and np.array_equal(s1, s2)
    assert np.isin(s1, x).all() and np.all(np.diff(s1) >= 0) and len(np.unique(s1)) > 32
    # pred + params + loss5 + grad_norm at their caps, with the .npy headers
    assert 4 * (bench.DUMP_PRED_ELEMS + bench.DUMP_PARAM_ELEMS + 5 + 1) + 4 * 128 <= 64e6


@pytest.mark.gpu
def test_plain_run_dumps_last_step(cad, dev, tmp_path):
    import torch
    from cad_amd import synthetic
    t = TINY
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", t["steps"], "--warmup", t["warmup"],
           "--batch", t["batch"], "--height", t["height"], "--width", t["width"], "--features", t["features"],
           "--dump-outputs", out_dir]
    r = subprocess.run(list(map(str, cmd)), capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["full"] is False and out["steps"] == t["steps"] and out["warmup"] == t["warmup"]
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "fp32"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(1e3 * t["batch"] / out["ms_per_step"], rel=1e-3)
    for leg in ("roofline", "cpu_baseline", "parity", "bf16_workloads", "data_path"):
        assert out[leg] is None, leg
    assert sorted(os.listdir(out_dir)) == ["grad_norm.npy", "loss5.npy", "params.npy", "pred.npy"]
    got = {n[:-4]: np.load(out_dir / n) for n in os.listdir(out_dir)}
    assert all(a.dtype == np.float32 for a in got.values())
    assert out["dumped_outputs"] == {n: list(a.shape) for n, a in got.items()}

    # the same steps here: bench.py's set-up at this shape
    lib = cad.load_library()
    prev = lib.cad_get_gemm_engine()
    assert lib.cad_set_gemm_engine(1) == 0
    try:
        B, H, W, f = t["batch"], t["height"], t["width"], t["features"]
        model = cad.BaselineUNet(3, f, max_depth=10.0, batch=B, height=H, width=W, device=dev.index)
        loss = cad.CombinedDepthLoss(1.0, 0.0, 0.0, 0.0, batch=B, height=H, width=W, device=dev.index)
        trainer = cad.Trainer(model, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
        rgb, gt, K = (x.to(dev) for x in synthetic.device_batch(B, H, W, "cpu"))
        for _ in range(t["warmup"] + t["steps"]):
            loss5 = trainer.train_step(rgb, gt, K)
        torch.cuda.synchronize(dev)
        assert got["pred"].shape == (B, 1, H, W) and np.array_equal(got["pred"], trainer.pred.cpu().numpy())
        assert np.array_equal(got["loss5"], loss5.cpu().numpy())
        assert got["loss5"][0] == np.float32(out["last_loss"])
        assert got["grad_norm"][0] == np.float32(model.last_grad_norm())
        params = np.concatenate([v.numpy().reshape(-1) for v in model.named_parameters().values()])
        assert params.size == out["config"]["params"] <= _bench().DUMP_PARAM_ELEMS   # stored whole
        assert np.array_equal(got["params"], params)
    finally:
        lib.cad_set_gemm_engine(prev)
