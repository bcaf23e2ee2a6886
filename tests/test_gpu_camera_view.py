"""The virtual-camera warp on the GPU (csrc/kernels/view_kernels.hip, cad_camera_view / cad_view_resolve) against
tests/camera_view_restatement.py, its exactness cases and refusals, the camera sweep of cad.evaluate and of
build/evaluate.

Shapes: one pixel; one row / column pair thinner than a bilinear cell; a batch smaller than a wave; (3, 33, 65) with
three different views in one batch, one of them the identity (odd sizes, more than one block per sample); and
520 x 520, just above the 1024 x 256 = 262144 pixels one pass of the launch covers, so the grid-stride loop runs
a second time for part of the grid.

Bounds.  delta = 8 x DEV is test_camera_view_cpu.py's (DEV: the measured fp32 - fp64 coordinate deviation, 1e-5 px
up to 65 wide, 1e-4 px above).
  rgb    bilinear interpolation is continuous and piecewise linear with slopes at most Gx = max |rgb(y, x+1) -
         rgb(y, x)| and Gy likewise, and clamping the coordinate does not stretch it, so a coordinate off by at most
         delta in u and in v moves the value by at most delta (Gx + Gy).  The lerp itself is three levels of a product
         pair and a sum on weights 1 - l and l (l = u - floor u is exact, 1 - l rounds once): 8 x 2^-24 x max |rgb|
         covers its roundings.  Compared at every pixel.
  depth  on the safe pixels (u + 0.5 and v + 0.5 further than delta from an integer, |d.z| > delta) the device must
         pick the restatement's tap, so valid is equal and Z' = Z / d.z agrees with the fp32 quotient to 1 ulp.  At
         least 98 % of the pixels of every case are safe (asserted).
  K'     bit for bit.
Measured on the MI355X (printed by test_against_restatement), largest over the views of a shape, masked or not:

    shape          rgb error   bound     kept      valid flips over all pixels   depth ulps
    (1, 1, 1)      0           4.3e-7    100 %     0                             0
    (1, 2, 9)      2.9e-7      1.4e-4    100 %     0                             0
    (1, 9, 2)      2.4e-7      1.4e-4    100 %     0                             0
    (2, 5, 7)      3.3e-7      1.5e-4    100 %     0                             0
    (3, 33, 65)    3.6e-6      1.6e-4    99.98 %   0                             0
    (1, 520, 520)  6.1e-5      1.6e-3    99.68 %   0                             0

The device's fp32 coordinates are the restatement's fp32 ones (no tap differs even outside the safe set, the quotient
is the same bits), so the rgb error is the fp32 - fp64 coordinate deviation times the image's slope, as derived.
"""
import csv
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

import camera_view_restatement as V
from conftest import ROOT
from test_camera_view_cpu import delta_for

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
SHAPES = ((1, 1, 1), (1, 2, 9), (1, 9, 2), (2, 5, 7), (3, 33, 65), (1, 520, 520))
VIEWS = (dict(zoom=0.7), dict(zoom=1.5, shift_x=0.11), dict(zoom_x=1.2, shift_y=-0.07), dict(yaw=7), dict(yaw=25, pitch=-5, roll=10))
KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "mae", "log10", "delta_1.25", "delta_1.25^2", "delta_1.25^3",
        "num_valid_pixels", "mean_pred_depth", "mean_gt_depth")


def _dev(arrs, dev):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def _lib_view(cad, view):
    return cad.view(**{k: v for k, v in view.items()})


def _ulp_diff(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check(shape, tag, got, rgb, depth, mask, K, Kn, R):
    """got = (rgb', depth', K', valid) device tensors of cad.camera_view against the restatement."""
    B, H, W = shape
    delta = delta_for(H, W)
    w = V.warp(rgb, depth, mask, K, Kn, R, delta)
    g_rgb, g_d, g_K, g_v = (t.cpu().numpy() for t in got)
    assert g_K.tobytes() == Kn.tobytes(), tag
    gx = np.abs(np.diff(rgb, axis=3)).max(initial=0.0)
    gy = np.abs(np.diff(rgb, axis=2)).max(initial=0.0)
    bound = delta * (gx + gy) + 8 * 2.0 ** -24 * np.abs(rgb).max()
    rgb_err = np.abs(g_rgb.astype(np.float64) - w["rgb"]).max()
    safe, share = w["safe"], w["safe"].mean()
    flips = int((g_v != w["valid"]).sum())                       # how many pixels the safe mask had to cover
    both = safe & w["valid"] & g_v
    ulps = int(_ulp_diff(g_d[both], w["depth"][both]).max(initial=0))
    print(f"{shape} {tag}: rgb error {rgb_err:.3g} (bound {bound:.3g}), kept {100 * share:.2f} %, valid flips over all "
          f"pixels {flips}, depth ulps {ulps}")
    assert rgb_err <= bound, tag
    assert share >= 0.98, tag
    assert np.array_equal(g_v[safe], w["valid"][safe]), tag
    assert ulps <= 1, tag
    warped = np.array([not i for i in w["identity"]])   # (an identity sample is a copy: its holes keep their bits)
    assert np.all(g_d[warped][(safe & ~w["valid"])[warped]] == 0), tag
    assert np.all((g_d[warped] != 0) == g_v[warped]), tag   # depth 0 is exactly the holes
    for b, ident in enumerate(w["identity"]):
        if ident:
            assert g_rgb[b].tobytes() == rgb[b].tobytes() and g_d[b].tobytes() == depth[b].tobytes(), tag
    return w


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_restatement(cad, dev, shape, masked):
    B, H, W = shape
    rgb, depth, mask, K = V.synth(B, H, W)
    mask = mask if masked else None
    t_rgb, t_d, t_m, t_K = _dev((rgb, depth, mask, K), dev)
    views = VIEWS[1::3] if H * W > 10000 else VIEWS
    for view in views:
        full = V.make_view(**view)
        Kn, R = V.resolve(full, K, H, W)
        got_K, got_R = cad.resolve_view(_lib_view(cad, view), t_K, H, W)
        assert got_K.cpu().numpy().tobytes() == Kn.tobytes() and got_R.cpu().numpy().tobytes() == R.tobytes(), view
        _check(shape, str(view), cad.camera_view(t_rgb, t_d, t_K, view=_lib_view(cad, view), mask=t_m), rgb, depth, mask, K, Kn, R)
    if B == 3:   # three different views in one batch, one of them the identity
        per = [V.resolve(V.make_view(**v), K[b:b + 1], H, W) for b, v in enumerate((VIEWS[1], {}, VIEWS[4]))]
        Kn, R = np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per])
        t_Kn, t_R = _dev((Kn, R), dev)
        w = _check(shape, "mixed", cad.camera_view(t_rgb, t_d, t_K, K_new=t_Kn, R=t_R, mask=t_m), rgb, depth, mask, K, Kn, R)
        assert w["identity"] == [False, True, False]


def test_exactness(cad, dev):
    B, H, W = 2, 33, 65
    rgb, depth, mask, K = V.synth(B, H, W)
    t_rgb, t_d, t_m, t_K = _dev((rgb, depth, mask, K), dev)
    # the neutral view: every bit of rgb and depth (NaN, Inf and negative pixels included), K' == K
    for m in (None, t_m):
        o_rgb, o_d, o_K, o_v = cad.camera_view(t_rgb, t_d, t_K, view=cad.view(), mask=m)
        assert o_rgb.cpu().numpy().tobytes() == rgb.tobytes() and o_d.cpu().numpy().tobytes() == depth.tobytes()
        assert o_K.cpu().numpy().tobytes() == K.tobytes()
        assert np.array_equal(o_v.cpu().numpy(), V.source_valid(depth, None if m is None else mask))
    o2 = cad.camera_view(t_rgb, t_d, t_K)   # no view, no K_new, no R: the same
    assert o2[0].cpu().numpy().tobytes() == rgb.tobytes() and o2[1].cpu().numpy().tobytes() == depth.tobytes()
    # R = I, another K': d.z == 1, the depth keeps the bits of the sampled pixel
    view = dict(zoom=1.5, shift_x=0.11)
    Kn, R = V.resolve(V.make_view(**view), K, H, W)
    w = V.warp(rgb, depth, None, K, Kn, R, delta_for(H, W))
    o_d = cad.camera_view(t_rgb, t_d, t_K, view=cad.view(**view))[1].cpu().numpy()
    pick = w["safe"] & w["valid"]
    assert pick.mean() > 0.5 and o_d[pick].tobytes() == w["depth"][pick].tobytes()
    assert set(np.unique(o_d[o_d != 0]).tolist()) <= set(np.unique(depth[np.isfinite(depth)]).tolist())
    # zoom 0.5 about the image centre: a border of depth 0 and valid 0, rgb edge-replicated there
    rgb2, depth2, _, K2 = V.synth(1, H, W, bad=False)
    depth2[depth2 == 0] = 1.0
    K2[0, 0, 2], K2[0, 1, 2] = (W - 1) / 2, (H - 1) / 2
    o_rgb, o_d, _, o_v = (t.cpu().numpy() for t in cad.camera_view(*_dev((rgb2, depth2, K2), dev), view=cad.view(zoom=0.5)))
    v = o_v[0, 0]
    assert v[H // 2, W // 2] and not (v[0].any() or v[-1].any() or v[:, 0].any() or v[:, -1].any()) and 0.2 < v.mean() < 0.3
    assert np.all(o_d[0, 0][~v] == 0) and np.all(o_d[0, 0][v] > 0)
    assert o_rgb[0, :, 0, 0].tobytes() == rgb2[0, :, 0, 0].tobytes() and o_rgb[0, :, -1, -1].tobytes() == rgb2[0, :, -1, -1].tobytes()
    assert o_rgb[0, :, 0, W // 2 - 3].tobytes() != rgb2[0, :, 0, 0].tobytes()   # the top edge follows the top row, not a corner
    # a camera turned away from everything it saw: d.z < 0 everywhere, nothing valid, nothing written but zeros
    t_R = torch.tensor(np.diag([-1.0, 1.0, -1.0]).astype(np.float32), device=dev).repeat(B, 1, 1)   # half a turn about y
    o_rgb, o_d, _, o_v = cad.camera_view(t_rgb, t_d, t_K, R=t_R)
    assert not o_v.any() and not o_d.any() and not o_rgb.any()


def test_refusals(cad, dev):
    B, H, W = 2, 5, 7
    rgb, depth, mask, K = V.synth(B, H, W, bad=False)
    t_rgb, t_d, t_m, t_K = _dev((rgb, depth, mask, K), dev)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    fresh = lambda: (torch.empty_like(t_rgb), torch.empty_like(t_d), valid)
    view = cad.view(zoom=1.5)
    # aliased outputs: the launch-level alias check refuses them, nothing is launched
    n = B * H * W
    in_rgb = t_rgb.view(-1)[n:2 * n].view(B, 1, H, W)   # a depth output inside the rgb input
    for out in ((t_rgb, fresh()[1], valid), (fresh()[0], t_d, valid), (fresh()[0], in_rgb, valid),
                (fresh()[0], fresh()[1], t_m.view(B, 1, H, W))):
        with pytest.raises(cad.CadError, match="alias"):
            cad.camera_view(t_rgb, t_d, t_K, view=view, mask=t_m, out=out)
    big = torch.empty(3 * n + 8, dtype=torch.float32, device=dev)
    with pytest.raises(cad.CadError, match="alias"):   # depth_out inside rgb_out
        cad.camera_view(t_rgb, t_d, t_K, view=view, out=(big[:3 * n].view(B, 3, H, W), big[2 * n:3 * n].view(B, 1, H, W), valid))
    assert t_rgb.cpu().numpy().tobytes() == rgb.tobytes() and t_d.cpu().numpy().tobytes() == depth.tobytes()
    # bad views
    for kw in (dict(zoom=0.0), dict(zoom_x=-1.0), dict(yaw=80.0), dict(roll=-120.0), dict(pitch=float("nan")), dict(shift_y=float("inf"))):
        with pytest.raises(ValueError, match="view: "):
            cad.camera_view(t_rgb, t_d, t_K, view=kw)
    with pytest.raises(ValueError, match="either view or"):
        cad.camera_view(t_rgb, t_d, t_K, view=view, R=t_K)
    with pytest.raises(ValueError, match="view must be"):
        cad.camera_view(t_rgb, t_d, t_K, view=1.5)
    # wrong dtypes or shapes
    for args in ((t_rgb.double(), t_d, t_K), (t_rgb, t_d.half(), t_K), (t_rgb, t_d, t_K.double()), (t_rgb[:, :2], t_d, t_K),
                 (t_rgb, t_d[:1], t_K), (t_rgb, t_d, t_K[:, :2]), (t_rgb.cpu(), t_d, t_K), (t_rgb, t_d[:, :, :4], t_K)):
        with pytest.raises(ValueError):
            cad.camera_view(*args, view=view)
    with pytest.raises(ValueError, match="K_new"):
        cad.camera_view(t_rgb, t_d, t_K, K_new=t_K[:1])
    with pytest.raises(ValueError, match="mask"):
        cad.camera_view(t_rgb, t_d, t_K, view=view, mask=t_m[:1])
    with pytest.raises(ValueError):
        cad.resolve_view(view, t_K.double(), H, W)
    with pytest.raises(cad.CadError, match="H = 0"):
        cad.resolve_view(view, t_K, 0, W)


# ---- the sweep in cad.evaluate ----
F, EB, EH, EW = 4, 2, 32, 48


def _net(cad, oracle, model):
    cls = cad.BaselineUNet if model == "baseline" else cad.IntrinsicsConditionedUNet
    net = cls(3, F, **({} if model == "baseline" else {"camera_dim": 4}), max_depth=10.0, batch=EB, height=EH, width=EW)
    state = dict(oracle.init_params(F, seed=3, model=model))
    state.update(oracle.init_buffers(F, model=model))
    net.load_state_dict(state)
    return net


@pytest.fixture(scope="module")
def batches(oracle, dev):
    return [tuple(_dev(oracle.synth_batch(EB, EH, EW, rgb_seed=0xC0FFEE + i, hole_seed=0xD3E7 + i), dev)) for i in range(2)]


def _forward(cad, net, rgb, K):
    return net.forward_cam(rgb, cad.camera_from_K(K)) if net.conditioned else net.forward(rgb)


@pytest.mark.parametrize("model", ["baseline", "film"])
@pytest.mark.parametrize("align", ["none", "median"])
def test_evaluate_sweep_matches_by_hand(cad, dev, oracle, batches, model, align):
    net = _net(cad, oracle, model)
    sweep = {"zoom": [0.7, 1.5], "yaw": [-7], "shift_x": [0.11]}
    res = cad.evaluate(net, batches, align=align, camera_sweep=sweep)
    plain = cad.evaluate(net, batches, align=align)
    assert "camera_sweep" not in plain and plain["per_sample"].tobytes() == res["per_sample"].tobytes()
    assert plain["summary"] == res["summary"] and res["forward_ms_per_image"] > 0
    assert [v["label"] for v in res["camera_sweep"]] == ["zoom:0.7", "zoom:1.5", "yaw:-7", "shift_x:0.11"]
    net.eval()
    for entry, (axis, value) in zip(res["camera_sweep"], (("zoom", 0.7), ("zoom", 1.5), ("yaw", -7), ("shift_x", 0.11))):
        view = cad.view(**{axis: value})
        assert entry["view"] == view.as_dict()
        ev = cad.Evaluator(2 * EB, EB, EH, EW, align=align)
        for rgb, gt, K in batches:
            rgb_v, gt_v, K_v, _ = cad.camera_view(rgb, gt, K, view=view)
            ev.update(_forward(cad, net, rgb_v, K_v), gt_v)
        assert entry["per_sample"].tobytes() == ev.metrics().tobytes(), entry["label"]
        assert entry["summary"] == ev.summary() and entry["alignment"].tobytes() == ev.alignment().tobytes()
        main_valid = sum(float(((b[1] > 0.1) & (b[1] < 10.0)).sum()) for b in batches)
        assert entry["valid_share"] == pytest.approx(ev.sums()[:, 0].sum() / main_valid, rel=1e-12)
        assert 0.2 < entry["valid_share"] < 1.2 and entry["per_sample"][:, 9].min() > 0
    assert res["camera_sweep"][0]["valid_share"] < 0.6   # zoom 0.7: about half of the pixels look at the image


def test_evaluate_neutral_view_and_view_intrinsics(cad, dev, oracle, batches):
    base = _net(cad, oracle, "baseline")
    views = [("neutral", cad.view()), ("zoom:1.5", cad.view(zoom=1.5))]
    res = cad.evaluate(base, batches, camera_sweep=views)
    assert res["camera_sweep"][0]["per_sample"].tobytes() == res["per_sample"].tobytes()
    assert res["camera_sweep"][0]["valid_share"] == 1.0
    masked = [b + ((b[1] > 2.0),) for b in batches]   # with a mask the neutral view still scores the main pass's pixels
    res_m = cad.evaluate(base, masked, camera_sweep=views[:1])
    assert res_m["camera_sweep"][0]["per_sample"].tobytes() == res_m["per_sample"].tobytes()
    assert res_m["per_sample"].tobytes() != res["per_sample"].tobytes()
    # BaselineUNet never sees K: the two settings are the same bits
    src = cad.evaluate(base, batches, camera_sweep=views, view_intrinsics="source")
    assert src["view_intrinsics"] == "source" and res["view_intrinsics"] == "true"
    for a, b in zip(res["camera_sweep"], src["camera_sweep"]):
        assert a["per_sample"].tobytes() == b["per_sample"].tobytes()
    # IntrinsicsConditionedUNet does: under zoom 1.5 they differ, under the neutral view K' is K
    film = _net(cad, oracle, "film")
    t = cad.evaluate(film, batches, camera_sweep=views)["camera_sweep"]
    s = cad.evaluate(film, batches, camera_sweep=views, view_intrinsics="source")["camera_sweep"]
    assert t[0]["per_sample"].tobytes() == s[0]["per_sample"].tobytes()
    assert t[1]["per_sample"].tobytes() != s[1]["per_sample"].tobytes()
    assert t[1]["per_sample"][:, 9].tobytes() == s[1]["per_sample"][:, 9].tobytes()   # the same warped ground truth
    with pytest.raises(ValueError, match="view_intrinsics"):
        cad.evaluate(base, batches, camera_sweep=views, view_intrinsics="both")
    with pytest.raises(ValueError, match="axis"):
        cad.evaluate(base, batches, camera_sweep={"tilt": [1]})


def _strip(report):
    """report.txt without the lines that differ from run to run (the date, the device time)."""
    return "\n".join(x for x in report.splitlines() if not x.startswith(("Evaluation Date:", "  Mean Time:", "  FPS:")))


def test_cli_camera_sweep(cad, dev, oracle, tmp_path):
    subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", "evaluate"], check=True, capture_output=True)
    n, bs = 6, 4
    net = cad.BaselineUNet(3, F, 10.0, batch=bs, height=EH, width=EW)
    state = dict(oracle.init_params(F, seed=5))
    state.update(oracle.init_buffers(F))
    net.load_state_dict(state)
    ck = tmp_path / "model.pt"
    cad.save(net, str(ck))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "train_config.yaml")))
    cfg["data"].update(num_train_samples=8, num_val_samples=n, input_height=EH, input_width=EW)
    cfg["model"]["init_features"] = F
    cfg["training"].update(batch_size=bs)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    exe = os.path.join(ROOT, "build", "evaluate")
    base = [exe, "-c", str(ck), "-g", str(p), "--align", "median"]
    out, out0 = tmp_path / "sweep", tmp_path / "plain"
    r = subprocess.run(base + ["-o", str(out), "--camera-sweep", "zoom:0.7,1.5", "--camera-sweep", "yaw:-7"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["-o", str(out0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # without the option: no new file; with it: the existing files keep their bytes, the report gains a section at its end
    assert sorted(f.name for f in out0.iterdir()) == ["per_sample.csv", "report.txt", "summary.csv"]
    assert sorted(f.name for f in out.iterdir()) == ["camera_sweep.csv", "per_sample.csv", "per_sample_camera.csv", "report.txt",
                                                     "summary.csv"]
    for name in ("per_sample.csv", "summary.csv"):
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    rep, rep0 = _strip((out / "report.txt").read_text()), _strip((out0 / "report.txt").read_text())
    assert "Camera Sweep" not in rep0 and rep.startswith(rep0) and "Camera Sweep" in rep[len(rep0):]
    for word in ("zoom", "yaw", "(unwarped)", "0.7", "1.5", "-7"):
        assert word in rep[len(rep0):], word
    # the files against cad.evaluate on the same checkpoint and the loader's batches
    seed = int(cfg.get("experiment", {}).get("seed", 42))
    ds = cad.SunRGBDDataset.synthetic(n, EH, EW, seed + 1)
    batches = [tuple(t.clone() for t in b[:3]) for b in cad.PrefetchLoader(ds, bs, EH, EW).epoch()]
    net2 = cad.BaselineUNet(3, F, 10.0, batch=bs, height=EH, width=EW)
    cad.load(net2, str(ck))
    res = cad.evaluate(net2, batches, align="median", camera_sweep={"zoom": [0.7, 1.5], "yaw": [-7]})
    rows = list(csv.DictReader(open(out / "per_sample_camera.csv")))
    assert list(rows[0]) == ["axis", "value", "index"] + list(KEYS) + ["scale", "shift", "aligned"] and len(rows) == 3 * n
    srows = list(csv.DictReader(open(out / "camera_sweep.csv")))
    assert list(srows[0])[:4] == ["axis", "value", "num_samples", "valid_share"] and len(srows) == 3
    assert list(srows[0])[4:] == list(csv.DictReader(open(out / "summary.csv")).fieldnames)[1:]
    for k, entry in enumerate(res["camera_sweep"]):
        axis, value = entry["label"].split(":")
        mine = [x for x in rows if (x["axis"], x["value"]) == (axis, value)]
        assert [int(x["index"]) for x in mine] == list(range(n))
        got = np.array([[np.float32(x[key]) for key in KEYS] for x in mine])
        assert got.tobytes() == entry["per_sample"].tobytes(), entry["label"]   # 9 digits carry an fp32 exactly
        assert np.array([[np.float32(x["scale"]), np.float32(x["shift"])] for x in mine]).tobytes() == entry["alignment"].tobytes()
        assert [int(x["aligned"]) for x in mine] == [int(a) for a in entry["aligned"]]
        s = srows[k]
        assert (s["axis"], s["value"], int(s["num_samples"])) == (axis, value, n)
        assert float(s["valid_share"]) == pytest.approx(entry["valid_share"], rel=1e-8)
        for stat in ("mean", "std", "median", "pooled"):
            assert [np.float32(s[f"{key}_{stat}"]) for key in KEYS] == [np.float32(entry["summary"][stat][key]) for key in KEYS], stat
    # --view-intrinsics source on a model that never sees K: the same tables
    out_s = tmp_path / "source"
    r = subprocess.run(base + ["-o", str(out_s), "--camera-sweep", "zoom:0.7,1.5", "--camera-sweep", "yaw:-7", "--view-intrinsics",
                               "source"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (out_s / "per_sample_camera.csv").read_bytes() == (out / "per_sample_camera.csv").read_bytes()
    assert "--view-intrinsics source" in (out_s / "report.txt").read_text()
    # and the long-form file feeds --compare --view
    r = subprocess.run([exe, "--compare", str(out / "per_sample_camera.csv"), str(out_s / "per_sample_camera.csv"), "--view", "zoom:1.5"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "abs_rel [zoom:1.5]" in r.stdout, r.stderr
