"""Geometric evaluation on the GPU (csrc/kernels/eval_geom_kernels.hip behind cad_evaluator_set_geometry,
cad_depth_normals and cad_exporter_normals) against the float64 NumPy restatement of
tests/eval_geom_restatement.py.

Tolerance (eval_geom_restatement.py, measured by test_eval_geom_cpu.py): numpy's fp32 form of the same
operations strays at most 2.23e-5 degrees per pixel from float64 on these inputs; the device gets 8 x the
recorded 2.3e-5, TOL_PIXEL = 1.84e-4 degrees, for FMA contraction and its own atan2f.  The inputs keep every
theta 1.84e-3 degrees from 11.25 / 22.5 / 30, so n_normal and the three counts are exact; sum theta is
within n TOL_PIXEL, sum theta^2 within the bound that follows from it, the point sums within 1e-6 / 2e-6
relative (ten fp32 roundings), the median within TOL_PIXEL.

Measured on the MI355X at these shapes: |sum theta - fp64| / n between 8e-8 and 9e-7 degrees, the median
within 1.6e-6 degrees of the restated one: two orders of magnitude inside the bound."""
import csv
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

import eval_align_restatement as A
import eval_geom_restatement as G
import eval_restatement as R
import eval_strata_restatement as S
import export_restatement as X
from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")


def _dev(arrs, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _run(cad, pred, gt, K, mask=None, clamp=True, splits=None, align="none", geometry=True, **kw):
    """-> (geometry sums, medians, total sums, evaluator)"""
    B, _, H, W = pred.shape
    ev = cad.Evaluator(B, B, H, W, clamp_pred=clamp, align=align, geometry=geometry, **kw)
    i = 0
    for n in splits or (B,):
        ev.update(pred[i:i + n], gt[i:i + n], None if mask is None else mask[i:i + n], K[i:i + n])
        i += n
    assert ev.count == B
    g = ev.geometry() if geometry else {"sums": None, "medians": None}
    return g["sums"], g["medians"], ev.sums(), ev


@pytest.mark.parametrize("config", G.CONFIGS, ids=lambda c: f"{c[3]}-{'masked' if c[1] else 'all'}-{'clamp' if c[2] else 'raw'}")
@pytest.mark.parametrize("shape", G.SHAPES)
def test_geometry_matches_restatement(cad, dev, shape, config):
    scaled, masked, clamp, mode = config
    pred, spred, gt, mask, K = G.make_inputs(*shape)
    pred, mask = spred if scaled else pred, mask if masked else None
    p, g, k = _dev((pred, gt, K), dev)
    m = None if mask is None else _dev((mask,), dev)[0]
    sums, med, total, ev = _run(cad, p, g, k, m, clamp, align=mode)
    # the restatement scores the evaluator's own (scale, shift) rows, which the alignment tests cover
    st = None if mode == "none" else ev.alignment()
    if st is not None:
        want_st = A.ref_alignment(mode, pred, gt, mask, G.LO, G.HI)[0]
        np.testing.assert_allclose(st, want_st, rtol=1e-5, atol=1e-6)
    w_sums, w_med, _, nv, n_valid = G.ref_geom(pred, gt, mask, K, G.LO, G.HI, clamp, st)
    assert sums.shape == (shape[0], 8) and med.shape == (shape[0],) and med.dtype == np.float32
    assert np.array_equal(total[:, 0], n_valid)
    G.assert_geom_close(sums, med, w_sums, w_med)
    if shape in ((1, 2, 9), (1, 9, 2)):   # no interior pixel: zeros, median 0, and the sample is counted
        assert not sums[:, :6].any() and med[0] == 0 and sums[0, 6] > 0 and ev.count == 1
    if shape == (1, 3, 3):
        assert sums[0, 0] == 1
    # the finished metrics
    geo = ev.geometry()
    np.testing.assert_allclose(geo["metrics"], G.finish(sums, med, total[:, 0]), rtol=1e-6)
    assert geo["summary"]["count"] == shape[0] and np.isnan(geo["summary"]["pooled"]["normal_median"])


def test_every_neighbour_pattern(cad, dev):
    """One hole in an otherwise complete image: the pixel itself and the pixels left / right / above / below it
    lose their normal (centre, right, left, down, up missing respectively), nothing else does."""
    pred, _, gt, _, K = G.make_inputs(1, 5, 7)
    mask = np.ones((1, 1, 5, 7), np.uint8)
    mask[0, 0, 2, 3] = 0
    p, g, m, k = _dev((pred, gt, mask, K), dev)
    sums, med, total, _ = _run(cad, p, g, k, m)
    full = _run(cad, p, g, k, None)[0]
    assert full[0, 0] == 15 and sums[0, 0] == 10 and total[0, 0] == 34
    w = G.ref_geom(pred, gt, mask, K)
    G.assert_geom_close(sums, med, w[0], w[1])
    _, valid = cad.depth_normals(g, k, m)
    want = np.ones((5, 7), bool)
    want[[0, -1], :] = want[:, [0, -1]] = False
    for r, c in ((2, 3), (2, 2), (2, 4), (1, 3), (3, 3)):
        want[r, c] = False
    assert np.array_equal(valid[0, 0].cpu().numpy(), want) and np.array_equal(w[3][0], want)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", G.SHAPES)
def test_depth_normals(cad, dev, shape, masked):
    _, _, gt, mask, K = G.make_inputs(*shape)
    d = gt.copy()
    if d.size >= 200:
        d.reshape(-1)[[5, 77, 150]] = [np.nan, np.inf, -1.0]
    g, m, k = _dev((d, mask, K), dev)
    nrm, valid = cad.depth_normals(g, k, m if masked else None)
    w_n, w_v = G.ref_normals(d, K, mask if masked else None)
    assert nrm.shape == (shape[0], 3) + shape[1:] and valid.shape == (shape[0], 1) + shape[1:] and valid.dtype == torch.bool
    assert np.array_equal(valid.cpu().numpy(), w_v)
    got = nrm.cpu().numpy().astype(np.float64)
    assert not got[~np.broadcast_to(w_v, got.shape)].any(), "zeros where invalid"
    # a unit vector off by angle t differs by 2 sin(t / 2) <= t: TOL_PIXEL in radians, plus the fp32 rounding of n
    tol = np.deg2rad(G.TOL_PIXEL) + 2.0 ** -23
    print("max |n - n64|", np.abs(got - w_n).max(), "bound", tol)
    assert np.abs(got - w_n).max() <= tol
    if w_v.any():
        ln = np.sqrt((got ** 2).sum(1, keepdims=True))[w_v]
        assert np.abs(ln - 1).max() < 1e-6 and (got[:, 2:3][w_v] < 0).all()
    # another range: the validity follows it
    nrm2, valid2 = cad.depth_normals(g, k, None, min_depth=2.5, max_depth=3.5)
    assert np.array_equal(valid2.cpu().numpy(), G.ref_normals(d, K, None, 2.5, 3.5)[1])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(3, 50, 70), (2, 16, 130)])
def test_existing_rows_untouched(cad, dev, shape, masked):
    """The total row and the strata rows are the same bits with geometry on and off; the geometry rows are the
    same bits with strata on and off."""
    pred, _, gt, mask, K = G.make_inputs(*shape)
    p, g, m, k = _dev((pred, gt, mask, K), dev)
    m = m if masked else None
    B, H, W = shape
    plain = cad.Evaluator(B, B, H, W)
    plain.update(p, g, m)
    gs, gm, tot, _ = _run(cad, p, g, k, m)
    assert tot.tobytes() == plain.sums().tobytes()
    kw = dict(depth_bins=S.DEPTH_CUTS, angle_bins=S.ANGLE_CUTS)
    s_off = _run(cad, p, g, k, m, geometry=False, **kw)[3]
    gs2, gm2, tot2, s_on = _run(cad, p, g, k, m, **kw)
    assert tot2.tobytes() == tot.tobytes() and gs2.tobytes() == gs.tobytes() and gm2.tobytes() == gm.tobytes()
    for axis in ("depth", "angle"):
        assert s_on.strata(axis)["sums"].tobytes() == s_off.strata(axis)["sums"].tobytes()
    for mode in ("median", "scale_shift"):
        a = cad.Evaluator(B, B, H, W, align=mode)
        a.update(p, g, m)
        _, _, t3, e3 = _run(cad, p, g, k, m, align=mode)
        assert t3.tobytes() == a.sums().tobytes() and e3.alignment().tobytes() == a.alignment().tobytes()


def _offset(t, elems):
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("masked", [False, True])
def test_aligned_and_offset_tensors_bit_identical(cad, dev, masked):
    pred, _, gt, mask, K = G.make_inputs(2, 64, 96)
    p, g, m, k = _dev((pred, gt, mask, K), dev)
    assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and m.data_ptr() % 4 == 0
    a = _run(cad, p, g, k, m if masked else None, align="median")
    po, go = _offset(p, 1), _offset(g, 1)
    assert po.data_ptr() % 16 == 4 and go.data_ptr() % 16 == 4
    b = _run(cad, po, go, k, m if masked else None, align="median")
    c = _run(cad, p, _offset(g, 2), k, _offset(m, 1) if masked else None, align="median")
    for i in range(3):
        assert a[i].tobytes() == b[i].tobytes() == c[i].tobytes(), i
    assert a[0][:, 0].min() > 1000


def test_batch_composition_invariance_and_determinism(cad, dev):
    pred, _, gt, mask, K = G.make_inputs(6, 50, 70)
    p, g, m, k = _dev((pred, gt, mask, K), dev)
    one = _run(cad, p, g, k, m, splits=(6,))
    three = _run(cad, p, g, k, m, splits=(1, 2, 3))
    six = _run(cad, p, g, k, m, splits=(1,) * 6)
    again = _run(cad, p, g, k, m, splits=(1, 2, 3))
    for i in range(3):
        assert one[i].tobytes() == three[i].tobytes() == six[i].tobytes() == again[i].tobytes(), i
    # each sample of the batch equals the sample evaluated alone (its own K row)
    alone = _run(cad, p[4:5], g[4:5], k[4:5], m[4:5])
    assert alone[0].tobytes() == one[0][4:5].tobytes() and alone[1].tobytes() == one[1][4:5].tobytes()
    w = G.ref_geom(pred, gt, mask, K)
    G.assert_geom_close(one[0], one[1], w[0], w[1])


def test_errors_leave_state_unchanged(cad, dev):
    pred, _, gt, mask, K = G.make_inputs(2, 16, 16)
    p, g, m, k = _dev((pred, gt, mask, K), dev)
    ev = cad.Evaluator(4, 2, 16, 16, geometry=True)
    assert ev.geometry_on
    ev.update(p, g, m, k)
    before = (ev.sums().tobytes(), ev.geometry()["sums"].tobytes(), ev.geometry()["medians"].tobytes())
    with pytest.raises(cad.CadError, match="K"):
        ev.update(p, g, m)                       # geometry is on: K is required
    assert ev.lib.cad_evaluator_update(ev.h, p.data_ptr(), g.data_ptr(), None, 2, None) == 1   # CAD_ERR_INVALID
    with pytest.raises(cad.CadError, match="count == 0"):
        ev.set_geometry(False)
    assert ev.count == 2 and ev.geometry_on
    assert (ev.sums().tobytes(), ev.geometry()["sums"].tobytes(), ev.geometry()["medians"].tobytes()) == before
    ev.update(p, g, m, k)                        # and the evaluator still works
    geo = ev.geometry()
    assert ev.count == 4 and geo["sums"][2:].tobytes() == geo["sums"][:2].tobytes() == before[1]
    ev.reset()
    ev.set_geometry(False)                       # allowed while empty; update without K works again
    ev.update(p, g, m)
    with pytest.raises(cad.CadError, match="off"):
        ev.geometry()
    off = cad.Evaluator(2, 2, 16, 16)
    off.update(p, g, m)
    with pytest.raises(cad.CadError, match="count == 0"):
        off.set_geometry(True)
    # the theta map may not be pred or gt: the alias guard refuses a pred inside the evaluator's scratch -- not
    # reachable through the API, so only the argument checks of the stand-alone entry points are exercised here
    lib = cad.load_library()
    assert lib.cad_depth_normals(None, k.data_ptr(), None, 2, 16, 16, 0.1, 10.0, None, None, None) == 1
    assert lib.cad_depth_normals(g.data_ptr(), k.data_ptr(), None, 2, 16, 16, 0.1, 10.0, None, None, None) == 1
    assert lib.cad_depth_normals(g.data_ptr(), k.data_ptr(), None, 2, 0, 16, 0.1, 10.0, g.data_ptr(), None, None) == 1


def test_update_allocates_nothing(cad, dev):
    pred, _, gt, mask, K = G.make_inputs(2, 16, 16)
    p, g, m, k = _dev((pred, gt, mask, K), dev)
    ev = cad.Evaluator(40, 2, 16, 16, geometry=True, align="median")
    st = torch.cuda.Stream(device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):   # the runtime builds a new stream's hardware queue at its first launch
        ev.update(p, g, m, k)
    ev.reset()
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    with torch.cuda.stream(st):
        e0.record()
        for _ in range(20):
            ev.update(p, g, m, k)
        e1.record()
    free1 = torch.cuda.mem_get_info(dev)[0]
    e1.synchronize()
    assert free0 == free1 == torch.cuda.mem_get_info(dev)[0]
    assert ev.count == 40 and e0.elapsed_time(e1) >= 0
    with torch.cuda.stream(st):
        geo = ev.geometry()
    assert all(geo["sums"][i].tobytes() == geo["sums"][i % 2].tobytes() and geo["medians"][i] == geo["medians"][i % 2]
               for i in range(40))
    ref = _run(cad, p, g, k, m, align="median")
    assert geo["sums"][:2].tobytes() == ref[0].tobytes() and geo["medians"][:2].tobytes() == ref[1].tobytes()


def test_predictor_normals(cad, dev):
    """A rendered plane gives the colour of its normal; a hole's neighbours and the border get `invalid`."""
    B, H, W = 2, 32, 80
    K = G.make_K(B, H, W)
    n1 = np.array([np.tan(np.deg2rad(25.0)), np.tan(np.deg2rad(-10.0)), -1.0])
    n1 /= np.linalg.norm(n1)
    d = np.stack([np.full((H, W), 2.5), G.plane_depth(n1, -3.0, K[1], H, W)])[:, None].astype(np.float32)
    d[1, 0, 7, 65] = 0.0      # holes: not positive, not finite
    d[0, 0, 11, 63] = np.nan
    mask = np.ones((B, 1, H, W), np.uint8)
    mask[0, 0, 3, 3] = 0
    t, k, m = _dev((d, K, mask), dev)
    net = cad.BaselineUNet(3, 4, 10.0, batch=B, height=H, width=W)
    pr = cad.Predictor(net, B, H, W)
    got = pr.normals(t, k, mask=m, invalid=(9, 8, 7)).cpu().numpy()
    assert got.shape == (B, H, W, 3) and got.dtype == np.uint8
    w_n, w_v = G.ref_normals(np.where(np.isfinite(d), d, 0), K, mask, 0.0, np.inf)
    want = G.normal_rgb(np.moveaxis(w_n, 1, -1))
    want[~w_v[:, 0]] = (9, 8, 7)
    assert (got[0, 1:-1, 1:-1][w_v[0, 0, 1:-1, 1:-1]] == (128, 128, 255)).all()
    for r, c in ((3, 3), (3, 2), (3, 4), (2, 3), (4, 3), (11, 63), (11, 64), (10, 63), (0, 0), (H - 1, 5), (5, W - 1)):
        assert tuple(got[0, r, c]) == (9, 8, 7), (r, c)
    assert tuple(got[1, 7, 64]) == (9, 8, 7) and tuple(got[1, 7, 66]) == (9, 8, 7)
    # the tilted plane: one colour, that of n1 (a colour step from fp32 rounding is allowed: +-1)
    inner = got[1][w_v[1, 0]].astype(int)
    assert np.abs(inner - G.normal_rgb(n1).astype(int)).max() <= 1 and np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert (got == want).mean() > 0.99
    # into a pane of a wider panel: the other columns stay untouched
    panel = torch.full((B, H, 2 * W + 3, 3), 200, dtype=torch.uint8, device=dev)
    pr.normals(t, k, mask=m, invalid=(9, 8, 7), out=panel, col_offset=W + 3)
    pn = panel.cpu().numpy()
    assert (pn[:, :, :W + 3] == 200).all() and np.array_equal(pn[:, :, W + 3:], got)


# ---------------- build/evaluate --geometry, build/predict --normals ----------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One epoch of build/train on the synthetic dataset at 32 x 48, as test_gpu_eval_strata.py's CLI test."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for target in ("train", "evaluate", "predict"):
        subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", target], check=True, capture_output=True)
    tmp = tmp_path_factory.mktemp("geom_cli")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_config.yaml")))
    cfg["data"].update(num_train_samples=16, num_val_samples=8, input_height=32, input_width=48)
    cfg["model"]["init_features"] = 8
    cfg["training"].update(num_epochs=1, batch_size=4)
    cfg["checkpointing"]["checkpoint_dir"] = str(tmp / "ckpt")
    cfg["logging"]["log_dir"] = str(tmp / "logs")
    p = tmp / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([os.path.join(ROOT, "build", "train"), "-c", str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return cfg, p, tmp / "ckpt" / "baseline_unet" / "final_model.pt", tmp


def test_cli_evaluate_geometry(cad, dev, trained):
    cfg, cfg_path, ckpt, tmp = trained
    exe = os.path.join(ROOT, "build", "evaluate")
    H, W = 32, 48
    outs = {}
    for name, opts in (("plain", []), ("geom", ["--geometry"]), ("geom_med", ["--geometry", "--align", "median"]),
                       ("geom_strata", ["--geometry", "--depth-bins", "1,2,3,5"]), ("strata", ["--depth-bins", "1,2,3,5"])):
        outs[name] = tmp / name
        r = subprocess.run([exe, "-c", str(ckpt), "-g", str(cfg_path), "-o", str(outs[name]), *opts], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    names = lambda d: sorted(f.name for f in d.iterdir())   # noqa: E731
    assert names(outs["plain"]) == ["per_sample.csv", "report.txt", "summary.csv"]
    assert names(outs["geom"]) == ["per_sample.csv", "per_sample_geometry.csv", "report.txt", "summary.csv", "summary_geometry.csv"]
    # the existing files keep their bytes (the report carries a date and a time: compare it without them)
    body = lambda d: [ln for ln in (d / "report.txt").read_text().splitlines()   # noqa: E731
                      if not ln.startswith(("Evaluation Date", "  Mean Time", "  FPS"))]
    for f in ("per_sample.csv", "summary.csv"):
        assert (outs["geom"] / f).read_bytes() == (outs["plain"] / f).read_bytes()
    for f in ("per_sample.csv", "summary.csv", "strata_depth.csv", "per_sample_strata.csv"):
        assert (outs["geom_strata"] / f).read_bytes() == (outs["strata"] / f).read_bytes()
    assert (outs["geom_strata"] / "per_sample_geometry.csv").read_bytes() == (outs["geom"] / "per_sample_geometry.csv").read_bytes()
    rep = body(outs["geom"])
    at = next(i for i, ln in enumerate(rep) if ln.strip() == "Geometric Metrics")
    assert rep[:at - 1] == body(outs["plain"])[:-1] and "Geometric Metrics" not in (outs["plain"] / "report.txt").read_text()
    assert any(ln.startswith("  < 11.25°:") for ln in rep[at:]) and any(ln.startswith("  MAE:") for ln in rep[at:])

    # the same model through cad.evaluate
    f = int(cfg["model"]["init_features"])
    max_depth = float(cfg["model"].get("max_depth", 10.0))
    net = cad.BaselineUNet(3, f, max_depth, batch=4, height=H, width=W)
    cad.load(net, str(ckpt))
    seed = int(cfg.get("experiment", {}).get("seed", 42))
    ds = cad.SunRGBDDataset.synthetic(8, H, W, seed + 1)
    batches = [tuple(t.clone() for t in b[:3]) for b in cad.PrefetchLoader(ds, 4, H, W).epoch()]
    for name, align in (("geom", "none"), ("geom_med", "median")):
        res = cad.evaluate(net, batches, max_depth=max_depth, align=align, geometry=True)
        geo = res["geometry"]
        rows = list(csv.DictReader(open(outs[name] / "per_sample_geometry.csv")))
        assert len(rows) == 8 and list(rows[0]) == ["index"] + list(G.KEYS)
        got = np.array([[np.float32(row[k]) for k in G.KEYS] for row in rows], np.float32)
        assert got.tobytes() == geo["metrics"].tobytes()
        assert (geo["sums"][:, 0] > 0).all() and (geo["metrics"][:, 7] > 0).all()
        summ = {row["statistic"]: row for row in csv.DictReader(open(outs[name] / "summary_geometry.csv"))}
        assert list(summ) == ["mean", "std", "median", "min", "max", "pooled"] and summ["pooled"]["normal_median"] == ""
        for stat in ("mean", "std", "median", "min", "max"):
            assert [np.float32(summ[stat][k]) for k in G.KEYS] == [np.float32(geo["summary"][stat][k]) for k in G.KEYS]
        assert np.float32(summ["pooled"]["point_mae"]) == np.float32(geo["summary"]["pooled"]["point_mae"])
        assert "geometry" not in cad.evaluate(net, batches, max_depth=max_depth, align=align)
    # alignment changes the point error, and the normals with it only through the clamp
    a = (outs["geom"] / "per_sample_geometry.csv").read_text()
    assert a != (outs["geom_med"] / "per_sample_geometry.csv").read_text()
    # --compare reads the geometry file by column name
    r = subprocess.run([exe, "--compare", str(outs["geom"] / "per_sample_geometry.csv"),
                        str(outs["geom_med"] / "per_sample_geometry.csv"), "--metric", "point_mae"], capture_output=True, text=True)
    assert r.returncode == 0 and "point_mae" in r.stdout and "t-statistic" in r.stdout, r.stderr
    r = subprocess.run([exe, "--compare", str(outs["geom"] / "per_sample_geometry.csv"),
                        str(outs["geom_med"] / "per_sample_geometry.csv")], capture_output=True, text=True)
    assert r.returncode == 1 and "abs_rel" in r.stderr and "normal_mean" in r.stderr


def test_cli_predict_normals(cad, dev, trained):
    cfg, cfg_path, ckpt, tmp = trained
    exe = os.path.join(ROOT, "build", "predict")
    H, W = 32, 48
    out = tmp / "pred_normals"
    r = subprocess.run([exe, "-c", str(ckpt), "-g", str(cfg_path), "-o", str(out), "--split", "val", "--indices", "0,5",
                        "--normals", "--npy"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert sorted(f.name for f in out.iterdir()) == ["predictions.csv", "val_0.npy", "val_0_normal.png", "val_5.npy",
                                                     "val_5_normal.png"]
    seed = int(cfg.get("experiment", {}).get("seed", 42))
    ds = cad.SunRGBDDataset.synthetic(8, H, W, seed + 1)
    K = next(iter(cad.PrefetchLoader(ds, 8, H, W).epoch()))[2]
    net = cad.BaselineUNet(3, int(cfg["model"]["init_features"]), 10.0, batch=1, height=H, width=W)
    pr = cad.Predictor(net, 1, H, W)
    for i in (0, 5):
        img = X.read_png((out / f"val_{i}_normal.png").read_bytes())
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        pred = torch.from_numpy(np.load(out / f"val_{i}.npy")[None, None]).to(dev)
        want = pr.normals(pred, K[i:i + 1].contiguous())
        assert np.array_equal(img, want[0].cpu().numpy())
        assert (img[0] == 0).all() and (img[:, 0] == 0).all() and img[1:-1, 1:-1].any()
    # files without intrinsics: refused before any device work, like --ply
    jpg = os.path.join(ROOT, "tests", "golden", "jpeg", "yuv420_96x128_restart_rows.jpg")
    r = subprocess.run([exe, "-c", str(ckpt), "-g", str(cfg_path), "-o", str(tmp / "none"), "-i", jpg, "--normals", "--dry-run"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--normals needs the camera" in r.stderr and not (tmp / "none").exists()
