"""Scale-aligned evaluation without a GPU: the restatement of tests/eval_align_restatement.py against
literal NumPy / torch operations (np.median, exp(mean(log)), torch.linalg.lstsq in float64), the host
solve cad_eval_solve_alignment (the code the device solve kernel runs) against the restatement in every
mode and every fallback, analytic cases, argument validation without a device, and build/evaluate's
--align flag."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import eval_align_restatement as A
import eval_restatement as R
from conftest import GOLDEN, ROOT

PKG = os.path.join(ROOT, "camera-aware-neural-networks-for-few-view-depth-estimation_amd")
EVALUATE = os.path.join(ROOT, "build", "evaluate")
CKPT = os.path.join(GOLDEN, "ckpt_baseline_f4", "baseline_unet_epoch_1.pt")
CFG = os.path.join(ROOT, "configs", "train_config.yaml")
SHAPES = ((1, 5, 7), (2, 16, 16), (3, 50, 70), (2, 64, 96))
MODE_ID = {"none": 0, "median": 1, "log_mean": 2, "scale_shift": 3}


@pytest.fixture(scope="module")
def evaluate_bin():
    subprocess.run(["make", "-C", PKG, "-o", "libcad_hip.so", "evaluate"], check=True, capture_output=True)
    return EVALUATE


def _solve(lib, mode, stats, med):
    st = np.ascontiguousarray(stats, np.float64)
    md = np.ascontiguousarray(med, np.float32)
    out = np.zeros(2, np.float32)
    rc = lib.cad_eval_solve_alignment(MODE_ID[mode], st.ctypes.data_as(C.POINTER(C.c_double)),
                                      md.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, lib.cad_last_error()
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_matches_literal_operations(shape):
    import torch
    pred, gt, mask = A.make_inputs(*shape)
    for lo, hi in R.RANGES:
        for m in (None, mask):
            med = A.ref_medians(pred, gt, m, lo, hi)
            for mode in A.MODES:
                st, ok = A.ref_alignment(mode, pred, gt, m, lo, hi)
                for b in range(shape[0]):
                    v = A.valid(gt[b], None if m is None else m[b], lo, hi)
                    p, g = pred[b].reshape(-1)[v], gt[b].reshape(-1)[v]
                    if p.size == 0:
                        assert tuple(st[b]) == (1.0, 0.0) and (mode == "none" or not ok[b])
                        continue
                    assert med[b, 0].tobytes() == np.median(p).astype(np.float32).tobytes()   # np.median of float32
                    assert med[b, 1].tobytes() == np.median(g).astype(np.float32).tobytes()
                    if mode == "none":
                        want = (np.float32(1), np.float32(0))
                    elif mode == "median":
                        want = (np.float32(np.median(g) / np.median(p)), np.float32(0)) if np.median(p) > 0 else (1, 0)
                    elif mode == "log_mean":
                        pos = p > 0
                        want = (np.float32(np.exp(np.mean(np.log(g[pos].astype(np.float64)) - np.log(p[pos].astype(np.float64))))),
                                np.float32(0))
                    else:
                        X = torch.stack([torch.from_numpy(p.astype(np.float64)), torch.ones(p.size, dtype=torch.float64)], 1)
                        sol = torch.linalg.lstsq(X, torch.from_numpy(g.astype(np.float64))[:, None]).solution[:, 0]
                        want = (np.float32(sol[0].item()), np.float32(sol[1].item()))
                    print(shape, lo, m is not None, mode, b, st[b], want)
                    assert A.ulp_diff(st[b, 0], want[0]) <= 2, (mode, st[b], want)
                    if mode == "scale_shift":   # the shift is a difference of order-1 terms: 2 ulp of their size
                        assert abs(float(st[b, 1]) - float(want[1])) <= 2 * 2.0 ** -23 * max(abs(float(want[1])), g.mean())
                    else:
                        assert st[b, 1] == want[1]
                    assert ok[b]


@pytest.mark.parametrize("mode", A.MODES)
def test_host_solve_matches_restatement(cad, mode):
    lib = cad.load_library()
    for shape in SHAPES:
        pred, gt, mask = A.make_inputs(*shape)
        for lo, hi in R.RANGES:
            for m in (None, mask):
                stats, med = A.ref_stats(pred, gt, m, lo, hi), A.ref_medians(pred, gt, m, lo, hi)
                want, _ = A.ref_alignment(mode, pred, gt, m, lo, hi)
                for b in range(shape[0]):
                    got = _solve(lib, mode, stats[b], med[b])
                    if mode in ("none", "median"):
                        assert got.tobytes() == want[b].tobytes(), (mode, got, want[b])
                    else:   # the same float64 formula; exp / rounding may differ in the last place
                        assert A.ulp_diff(got[0], want[b, 0]) <= 1 and abs(float(got[1]) - float(want[b, 1])) <= 2.0 ** -22


def test_host_solve_fallbacks(cad):
    lib = cad.load_library()
    one = np.array([1, 0], np.float32).tobytes()
    empty = np.zeros(7)
    for mode in A.MODES:   # no valid pixel
        assert _solve(lib, mode, empty, (0, 0)).tobytes() == one
    # median with med(pred) <= 0
    for mp in (0.0, -0.0, -2.5):
        assert _solve(lib, "median", [9, 4, 1, 20, 30, 5, 0], (mp, 3.0)).tobytes() == one
        assert A.solve("median", [9, 4, 1, 20, 30, 5, 0], (mp, 3.0))[:2] == (1, 0)
    # log_mean without a positive prediction
    assert _solve(lib, "log_mean", [5, 0, -4, 9, 6, -7, 0], (0, 0)).tobytes() == one
    # scale_shift with a degenerate normal matrix: one pixel (n p^2 - p^2 = 0) and a constant prediction
    for n, p, g in ((1, 1.5, 3.0), (8, 2.0, 5.0)):
        st = [n, n, n * p, n * g, n * p * p, n * p * g, 0]
        got = _solve(lib, "scale_shift", st, (0, 0))
        assert got.tobytes() == np.array([np.float32(g / p), 0], np.float32).tobytes(), got
        assert A.solve("scale_shift", st, (0, 0)) == (np.float32(g / p), 0, False)
    # ... and all predictions zero
    assert _solve(lib, "scale_shift", [4, 0, 0, 9, 0, 0, 0], (0, 0)).tobytes() == one
    # bad arguments
    out = (C.c_float * 2)()
    assert lib.cad_eval_solve_alignment(7, empty.ctypes.data_as(C.POINTER(C.c_double)), None, out) == 1
    assert lib.cad_eval_solve_alignment(1, empty.ctypes.data_as(C.POINTER(C.c_double)), None, out) == 1
    assert lib.cad_eval_solve_alignment(3, None, None, out) == 1


def test_analytic_cases(cad):
    """pred = c gt gives s = 1/c in every scale-only mode; pred = (gt - b)/a gives (a, b) for scale_shift; to
    2 fp32 ulp.  c is a power of two and (a, b) are small dyadic numbers so that pred is exact in fp32."""
    lib = cad.load_library()
    rng = np.random.default_rng(11)
    gt = rng.uniform(0.5, 9.0, (1, 1, 24, 32)).astype(np.float32)
    for c in (0.25, 4.0, 0.015625):
        pred = (gt * np.float32(c)).astype(np.float32)
        stats, med = A.ref_stats(pred, gt)[0], A.ref_medians(pred, gt)[0]
        for mode in ("median", "log_mean", "scale_shift"):
            got = _solve(lib, mode, stats, med)
            assert A.ulp_diff(got[0], np.float32(1 / c)) <= 2, (mode, c, got)
            assert abs(float(got[1])) <= 2 * 2.0 ** -23 * 9.0, (mode, c, got)
    a, b = 2.0, 0.375
    gt = (np.round(gt * 256) / 256).astype(np.float32)   # 8 fractional bits: (gt - b) / a is exact
    pred = ((gt - np.float32(b)) / np.float32(a)).astype(np.float32)
    assert np.array_equal(pred.astype(np.float64) * a + b, gt.astype(np.float64))
    got = _solve(lib, "scale_shift", A.ref_stats(pred, gt)[0], (0, 0))
    assert A.ulp_diff(got[0], np.float32(a)) <= 2 and A.ulp_diff(got[1], np.float32(b)) <= 2, got


def test_argument_validation_without_device(cad):
    lib = cad.load_library()
    assert lib.cad_evaluator_set_alignment(None, 1) == 1 and lib.cad_last_error()
    assert lib.cad_evaluator_get_alignment(None) == 0
    out = (C.c_float * 2)()
    assert lib.cad_evaluator_alignment(None, out, None) == 1
    p = C.c_void_p(4096)   # never dereferenced: every call below fails its argument check first
    for args in ((None, p, None, 1, 8, 8, 0.1, 10.0, p), (p, None, None, 1, 8, 8, 0.1, 10.0, p),
                 (p, p, None, 1, 8, 8, 0.1, 10.0, None), (p, p, None, 0, 8, 8, 0.1, 10.0, p),
                 (p, p, None, 1, 0, 8, 0.1, 10.0, p), (p, p, None, 1, 8, -3, 0.1, 10.0, p),
                 (p, p, None, 1, 8, 8, 0.0, 10.0, p), (p, p, None, 1, 8, 8, 5.0, 5.0, p)):
        assert lib.cad_valid_medians(*args, None) == 1, args
        assert lib.cad_last_error()
    from cad_amd import _abi
    for bad in ("bogus", "", None, 1, "Median"):
        with pytest.raises(ValueError):
            _abi.eval_align_mode(bad)
    assert [_abi.eval_align_mode(m) for m in A.MODES] == [0, 1, 2, 3]


def test_python_rejects_bad_mode_before_any_device_call(cad):
    """The mode string is checked first: ValueError even where no device exists."""
    with pytest.raises(ValueError):
        cad.Evaluator(4, 2, 8, 8, align="bogus")
    with pytest.raises(ValueError):
        cad.depth_metrics_full(None, None, align="mean")
    with pytest.raises(ValueError):
        cad.evaluate(None, [(None, None, None)], align="bogus")


def test_evaluate_align_flag(evaluate_bin, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")   # any device call would fail
    r = subprocess.run([evaluate_bin, "-c", CKPT, "-g", CFG, "-o", str(tmp_path / "out"), "--align", "bogus"],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("Error: --align 'bogus'") and not (tmp_path / "out").exists()
    for mode in A.MODES:
        r = subprocess.run([evaluate_bin, "-c", CKPT, "-g", CFG, "-o", str(tmp_path / "out"), "--dry-run", "--align", mode],
                           capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout)["align"] == mode
    r = subprocess.run([evaluate_bin, "-c", CKPT, "-g", CFG, "--dry-run"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and json.loads(r.stdout)["align"] == "none"
    assert "--align" in subprocess.run([evaluate_bin, "--help"], capture_output=True, text=True).stdout


def test_compare_accepts_alignment_columns(evaluate_bin, tmp_path):
    """--compare pairs by the index column and finds the metric by name: files with the trailing scale,
    shift, aligned columns compare like files without them, also one of each kind."""
    gold = json.load(open(os.path.join(GOLDEN, "eval_stats.json")))
    pair, want = gold["pairs"]["effect_n40"], gold["expected"]["effect_n40"]

    def write(path, col, extra):
        rows = ["index," + ",".join(R.KEYS) + (",scale,shift,aligned" if extra else "")]
        for i, v in enumerate(col):
            row = f"{i}," + ",".join(repr(float(v)) if k == "abs_rel" else "0" for k in R.KEYS)
            rows.append(row + (f",{1.5 + i},0,{i % 2}" if extra else ""))
        path.write_text("\n".join(rows) + "\n")
    a, b, plain = tmp_path / "a.csv", tmp_path / "b.csv", tmp_path / "plain.csv"
    write(a, pair["a"], True)
    write(b, pair["b"], True)
    write(plain, pair["b"], False)
    for other in (b, plain):
        r = subprocess.run([evaluate_bin, "--compare", str(a), str(other), "--metric", "abs_rel"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert f"t-statistic: {want['t']:.4f} (df=39)" in r.stdout and f"W statistic: {want['W']:.4f}" in r.stdout
