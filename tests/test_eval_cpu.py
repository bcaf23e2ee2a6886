"""Offline evaluation without a GPU: the float64 restatement the GPU tests compare against is itself
checked against the reference's arithmetic (DepthMetrics::compute, src/evaluation/depth_metrics.h:40-88,
written out as literal fp32 torch CPU ops); build/evaluate's flags, errors, --dry-run and --compare; the
evaluator's argument validation and host-side summary; include/cad/eval_stats.hpp against SciPy's results
(tests/golden/eval_stats.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import eval_restatement as R
from conftest import GOLDEN, ROOT

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
EVALUATE = os.path.join(ROOT, "build", "evaluate")
CKPT = os.path.join(GOLDEN, "ckpt_baseline_f4", "baseline_unet_epoch_1.pt")
CFG = os.path.join(ROOT, "configs", "train_config.yaml")
SHAPES = ((1, 5, 7), (3, 50, 70), (2, 64, 96), (2, 16, 16))


@pytest.fixture(scope="module")
def evaluate_bin():
    # (-o libcad_hip.so: the library is never rebuilt here, as in test_cli.py::train_bin)
    subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", "evaluate"], check=True, capture_output=True)
    return EVALUATE


def _torch_reference(pred, gt, mask, lo, hi):
    """DepthMetrics::compute on one sample, op for op in fp32 torch (depth_metrics.h:54-85, 147-233)."""
    import torch
    p, g = torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy())
    m = (g > lo) & (g < hi)
    if mask is not None:
        m = m & torch.from_numpy(mask.copy()).to(torch.bool)
    pv, gv = p.masked_select(m), g.masked_select(m)
    if pv.numel() == 0:
        return np.zeros(12)
    pv = torch.clamp(pv, lo, hi)
    ratio = torch.max(pv / gv, gv / pv)
    th = [float(R.T1), float(R.T2), float(R.T3)]
    return np.array([
        (torch.abs(pv - gv) / gv).mean().item(),
        (torch.pow(pv - gv, 2) / gv).mean().item(),
        torch.sqrt(torch.pow(pv - gv, 2).mean()).item(),
        torch.sqrt(torch.pow(torch.log(pv) - torch.log(gv), 2).mean()).item(),
        torch.abs(pv - gv).mean().item(),
        torch.abs(torch.log10(pv) - torch.log10(gv)).mean().item(),
        (ratio < th[0]).to(torch.float32).mean().item(),
        (ratio < th[1]).to(torch.float32).mean().item(),
        (ratio < th[2]).to(torch.float32).mean().item(),
        float(pv.numel()), pv.mean().item(), gv.mean().item()], np.float64)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_matches_reference_arithmetic(shape):
    """The restatement agrees with the fp32 torch path to 1e-5 relative on the test inputs (which also
    shows that on these inputs the reference itself is inside the 2e-5 bound of the GPU tests), with the
    valid-pixel count and the three threshold counts exact."""
    pred, gt, mask = R.make_inputs(*shape)
    assert (gt == 0).any() and (pred <= 0).any() and (pred > 10).any()
    for lo, hi in R.RANGES:
        assert (gt == np.float32(lo)).any() and (gt == np.float32(hi)).any()
        for m in (None, mask):
            sums = R.ref_sums(pred, gt, m, lo, hi, True)
            want = R.finish(sums)
            for b in range(shape[0]):
                got = _torch_reference(pred[b], gt[b], None if m is None else m[b], lo, hi)
                n = sums[b, 0]
                assert got[9] == n
                for k in (6, 7, 8):   # fractions of exact counts
                    assert round(got[k] * n) == sums[b, 7 + k - 6], (k, got[k] * n, sums[b])
                for k in (0, 1, 2, 3, 4, 5, 10, 11):
                    print(shape, lo, m is not None, b, R.KEYS[k], got[k], want[b, k])
                    assert abs(got[k] - want[b, k]) <= 1e-5 * abs(want[b, k]), (R.KEYS[k], got[k], want[b, k])
    # the thresholds bite on both sides and the log error is of order 0.5, as the tolerance assumes
    full = R.finish(R.ref_sums(pred, gt, None, 0.1, 10.0, True).sum(0))[0]
    # (the 35-pixel shape is dominated by its six out-of-range predictions)
    assert 0 < full[6] < full[7] < full[8] < 1 and (pred.size < 512 or 0.3 < full[3] < 0.8)


def test_evaluate_help_and_missing_checkpoint(evaluate_bin, tmp_path):
    r = subprocess.run([evaluate_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--checkpoint" in r.stdout
    r = subprocess.run([evaluate_bin, "-c", str(tmp_path / "none.pt"), "-g", CFG], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error: Cannot open checkpoint")
    r = subprocess.run([evaluate_bin, "-g", CFG], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error:")
    r = subprocess.run([evaluate_bin, "--bogus"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error:" in r.stderr


def test_evaluate_dry_run_opens_no_device(evaluate_bin, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # any device call would fail
    r = subprocess.run([evaluate_bin, "-c", CKPT, "-g", CFG, "-o", str(tmp_path / "out"), "--split", "train", "--dry-run"],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout)
    assert plan["architecture"] == "baseline_unet" and plan["format"] == "torch" and plan["split"] == "train"
    assert plan["batches"] == -(-plan["samples"] // plan["batch_size"])
    assert not (tmp_path / "out").exists()


def test_evaluator_argument_validation_without_device(cad):
    lib = cad.load_library()
    from cad_amd import _abi
    h = C.c_void_p()
    ok = _abi.EvalConfig(0.1, 10.0, 1)
    for cap, mb, H, W, cfg in ((0, 1, 8, 8, ok), (4, 0, 8, 8, ok), (4, 1, 0, 8, ok), (4, 1, 8, -1, ok),
                               (4, 1, 8, 8, _abi.EvalConfig(0.0, 10.0, 1)), (4, 1, 8, 8, _abi.EvalConfig(2.0, 2.0, 1)),
                               (4, 1, 8, 8, _abi.EvalConfig(5.0, 1.0, 0))):
        assert lib.cad_evaluator_create(cap, mb, H, W, C.byref(cfg), 0, C.byref(h)) == 1, (cap, mb, H, W)
        assert lib.cad_last_error() and not h.value


@pytest.mark.parametrize("n", [1, 5, 6])
def test_eval_finish_summary_host(cad, n):
    """cad_eval_finish (host double arithmetic rounded to fp32) against NumPy: per-sample metrics, mean,
    population std, median (odd and even N), min, max, pooled; a row without valid pixels counts as zeros."""
    lib = cad.load_library()
    from cad_amd import _abi
    pred, gt, mask = R.make_inputs(6, 16, 16)
    sums = R.ref_sums(pred, gt, mask)[:n].copy()
    if n > 1:
        sums[1] = 0.0
    per = np.zeros((n, 12), np.float32)
    s = _abi.EvalSummary()
    assert lib.cad_eval_finish(sums.ctypes.data_as(C.POINTER(C.c_double)), n, per.ctypes.data_as(_abi.FP), C.byref(s)) == 0
    np.testing.assert_allclose(per, R.finish(sums), rtol=1e-6, atol=0)
    assert s.count == n
    for stat, want in R.summary(sums).items():
        np.testing.assert_allclose(np.array(list(getattr(s, stat))), want, rtol=1e-6, atol=1e-12, err_msg=stat)
    if n > 1:
        assert not per[1].any()


# ---- include/cad/eval_stats.hpp against SciPy (tests/golden/eval_stats.json) ----
@pytest.fixture(scope="module")
def stats_probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("eval_stats") / "eval_stats_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "eval_stats_probe.cpp")], check=True)
    return str(exe)


def _probe(exe, tmp_path, pair, seed):
    f = tmp_path / "pair.txt"
    f.write_text(f"{len(pair['a'])}\n" + " ".join(repr(x) for x in pair["a"]) + "\n" + " ".join(repr(x) for x in pair["b"]) + "\n")
    out = subprocess.run([exe, str(f), str(seed)], check=True, capture_output=True, text=True).stdout
    return {k: float(v) for k, v in (line.split() for line in out.strip().splitlines())}


@pytest.mark.parametrize("name", ["ties_n12", "effect_n40", "null_n40"])
def test_eval_stats_match_scipy(stats_probe, tmp_path, name):
    gold = json.load(open(os.path.join(GOLDEN, "eval_stats.json")))
    pair, want = gold["pairs"][name], gold["expected"][name]
    got = _probe(stats_probe, tmp_path, pair, 7)
    for k in ("t", "W", "cohens_d", "mean_diff"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])
    assert got["df"] == want["df"] and got["n_nonzero"] == want["n_nonzero"]
    for k in ("t_p", "w_p"):
        tol = 1e-4 * want[k] if want[k] < 1e-3 else 1e-6
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])
    # percentile bootstrap of the mean difference: holds the sample mean, reproducible per seed
    assert got["ci_lo"] <= want["mean_diff"] <= got["ci_hi"] and got["ci_lo"] < got["ci_hi"]
    again, other = _probe(stats_probe, tmp_path, pair, 7), _probe(stats_probe, tmp_path, pair, 8)
    assert (again["ci_lo"], again["ci_hi"]) == (got["ci_lo"], got["ci_hi"])
    assert (other["ci_lo"], other["ci_hi"]) != (got["ci_lo"], got["ci_hi"])


def _write_csv(path, col, index=None):
    rows = ["index," + ",".join(R.KEYS)]
    for i, v in enumerate(col):
        rows.append(f"{i if index is None else index[i]}," + ",".join(repr(float(v)) if k == "abs_rel" else "0" for k in R.KEYS))
    path.write_text("\n".join(rows) + "\n")


def test_evaluate_compare(evaluate_bin, tmp_path):
    gold = json.load(open(os.path.join(GOLDEN, "eval_stats.json")))
    pair, want = gold["pairs"]["effect_n40"], gold["expected"]["effect_n40"]
    a, b, short, shifted = (tmp_path / n for n in ("a.csv", "b.csv", "short.csv", "shifted.csv"))
    _write_csv(a, pair["a"])
    _write_csv(b, pair["b"])
    _write_csv(short, pair["b"][:-1])
    _write_csv(shifted, pair["b"], index=list(range(1, 41)))
    r = subprocess.run([evaluate_bin, "--compare", str(a), str(b), "--metric", "abs_rel"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Paired t-test" in r.stdout and "Wilcoxon Signed-Rank Test" in r.stdout and "Bootstrap" in r.stdout
    assert f"t-statistic: {want['t']:.4f} (df=39)" in r.stdout and f"W statistic: {want['W']:.4f}" in r.stdout
    r = subprocess.run([evaluate_bin, "--compare", str(a), str(short)], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error:")
    r = subprocess.run([evaluate_bin, "--compare", str(a), str(shifted)], capture_output=True, text=True)
    assert r.returncode == 1 and "indices" in r.stderr
    r = subprocess.run([evaluate_bin, "--compare", str(a), str(b), "--metric", "nope"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error:")
