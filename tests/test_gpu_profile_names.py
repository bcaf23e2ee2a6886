"""The launch profiler's kernel names are pinned (csrc/kernels/kernels.hpp KName, epilogues.hpp `name`).

bench.py takes the dominant kernel's name from the profiler census and hands it back through
cad_profile_only, and the saved profiles/ compare by name, so a refactor of the launchers must not move a
single byte of them.  Every case below runs operator entry points (or, for the epilogues that only a network
reaches — fp32 BN partials, bn-sums, the split store, the big-tile ConvT input gradient — one small training
step) with the in-library profiler on, and the exact set of names it reports must equal
tests/golden/profile_names.json.

The golden file is recorded from a build of the commit BEFORE the change under test, never from the code
under test: the C ABI is the same, so
    CAD_LIB=<parent build's .so> CAD_PROFILE_NAMES_RECORD=1 pytest tests/test_gpu_profile_names.py
rewrites it (see the file's "_comment").

Cases: every window block shape per engine (S3, with and without the weight twin; bf16 256 x 128, 512 x 64
and 256 x 96 tiles), one im2col shape per tile config (C41 / C22 / C14) per engine, the stats / bf16 /
activation / FiLM / split-store / bn-sums epilogues, ConvT on the big-tile and DMA paths, the dense forward's
add / mask / stats forms, the MX-fp8 launches, and split-K with no, one-level and two-level slab reduction.
Operand values do not matter here (the arithmetic is tests/test_gpu_ops.py's business): zeros.
"""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import ROOT
from test_gpu_ops import B1_WIN_SHAPES, CONVT_BF16_SHAPES, WGRAD_BF16_SHAPES, WIN_SHAPES

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "profile_names.json")
RECORD = os.environ.get("CAD_PROFILE_NAMES_RECORD") == "1"
ENGINES = {"f32": 0, "s3": 1, "bf16": 2}
# B, H, W, cin, cout: im2col on every engine (cin % 16 != 0 or no block width divides W), one per tile config
IM2COL = {"C41": (2, 16, 24, 4, 64), "C22": (1, 8, 12, 128, 256), "C14": (2, 3, 4, 64, 128)}
IM2COL_PS = {"C41": (2, 16, 24, 8, 64), "C22": (1, 8, 12, 128, 256), "C14": (2, 3, 4, 64, 128)}
# bf16 window tiles that test_gpu_ops.B1_WIN_SHAPES leaves out: 256 x 128 at CW 128, 512 x 64 at CW 64,
# 256 x 96 at CW 16 / 8
B1_WIN_MORE = [(1, 4, 128, 64, 128), (1, 8, 64, 64, 64), (1, 16, 16, 96, 96), (1, 32, 8, 96, 96)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _z(dev, *shape, bf16=False, u8=False):
    return torch.zeros(*shape, device=dev, dtype=torch.uint8 if u8 else torch.bfloat16 if bf16 else torch.float32)


def _ok(lib, st):
    assert st == 0, lib.cad_last_error()


# ---- the operator calls (one entry point each; shapes B, H, W, cin, cout) ----
def conv_f32(lib, dev, B, H, W, cin, cout, what=("fwd", "dgrad", "wgrad")):
    x, w, y = _z(dev, B, H, W, cin), _z(dev, cout, 3, 3, cin), _z(dev, B, H, W, cout)
    if "fwd" in what:
        _ok(lib, lib.cad_op_conv3x3_fwd(_p(x), cin, 0, cin, _p(w), cout, _p(y), cout, 0, B, H, W, _s()))
    if "dgrad" in what:
        _ok(lib, lib.cad_op_conv3x3_dgrad(_p(y), cout, _p(w), cin, _p(x), cin, B, H, W, _s()))
    if "wgrad" in what:
        _ok(lib, lib.cad_op_conv3x3_wgrad(_p(y), cout, _p(x), cin, 0, cin, _p(w), B, H, W, _s()))


def conv_act(lib, dev, B, H, W, cin, cout):
    """cad_op_conv3x3_fwd_act: BN + ReLU, then with FiLM"""
    x, w, y = _z(dev, B, H, W, cin), _z(dev, cout, 3, 3, cin), _z(dev, B, H, W, cout)
    sc, gb = _z(dev, cout), _z(dev, B, cout)
    for g in (None, gb):
        _ok(lib, lib.cad_op_conv3x3_fwd_act(_p(x), cin, 0, cin, _p(w), cout, _p(sc), _p(sc), _p(g), _p(g), _p(y), cout, 0,
                                            0, B, H, W, _s()))


def conv_ps(lib, dev, B, H, W, cin, cout):
    """cad_op_conv3x3_fwd_bf16 (fp32 / bf16 rows, with and without BN partials) and _dgrad_bf16 (fp32 / bf16)"""
    x, w, dz = _z(dev, B, H, W, cin, bf16=True), _z(dev, cout, 3, 3, cin), _z(dev, B, H, W, cout, bf16=True)
    for yb in (0, 1):
        y = _z(dev, B, H, W, cout, bf16=bool(yb))
        for stats in (0, 1):
            _ok(lib, lib.cad_op_conv3x3_fwd_bf16(_p(x), cin, 0, cin, _p(w), cout, _p(y), cout, 0, yb, stats, B, H, W, _s()))
        dx = _z(dev, B, H, W, cin, bf16=bool(yb))
        _ok(lib, lib.cad_op_conv3x3_dgrad_bf16(_p(dz), cout, cout, _p(w), cin, _p(dx), cin, yb, B, H, W, _s()))


def conv_ps_act(lib, dev, B, H, W, cin, cout):
    """cad_op_conv3x3_fwd_act_bf16: fp32 / bf16 rows x (BN + ReLU, + FiLM)"""
    x, w = _z(dev, B, H, W, cin, bf16=True), _z(dev, cout, 3, 3, cin)
    sc, gb = _z(dev, cout), _z(dev, B, cout)
    for yb in (0, 1):
        y = _z(dev, B, H, W, cout, bf16=bool(yb))
        for g in (None, gb):
            _ok(lib, lib.cad_op_conv3x3_fwd_act_bf16(_p(x), cin, 0, cin, _p(w), cout, _p(sc), _p(sc), _p(g), _p(g), _p(y),
                                                     cout, 0, yb, B, H, W, _s()))


def wgrad_ps(lib, dev, B, H, W, cin, cout, xcoff=0):
    ldx = xcoff + cin + 8 if xcoff else cin
    x, dz, dw = _z(dev, B, H, W, ldx, bf16=True), _z(dev, B, H, W, cout, bf16=True), _z(dev, cout, 3, 3, cin)
    _ok(lib, lib.cad_op_conv3x3_wgrad_bf16(_p(dz), cout, cout, _p(x), ldx, xcoff, cin, _p(dw), B, H, W, _s()))


def convT_f32(lib, dev, B, H, W, cin, cout):
    x, w, b = _z(dev, B, H, W, cin), _z(dev, cin, 2, 2, cout), _z(dev, cout)
    y = _z(dev, B, 2 * H, 2 * W, cout)
    _ok(lib, lib.cad_op_convT_fwd(_p(x), cin, _p(w), _p(b), cout, _p(y), cout, 0, B, H, W, _s()))
    _ok(lib, lib.cad_op_convT_dgrad(_p(y), cout, 0, cout, _p(w), cin, _p(x), B, H, W, _s()))
    _ok(lib, lib.cad_op_convT_wgrad(_p(x), cin, _p(y), cout, 0, cout, _p(w), B, H, W, _s()))


def convT_ps(lib, dev, B, H, W, cin, cout):
    x, w, b = _z(dev, B, H, W, cin, bf16=True), _z(dev, cin, 2, 2, cout), _z(dev, cout)
    y = _z(dev, B, 2 * H, 2 * W, cout, bf16=True)
    _ok(lib, lib.cad_op_convT_fwd_bf16(_p(x), cin, 0, cin, _p(w), _p(b), cout, _p(y), cout, 0, B, H, W, _s()))


def dense(lib, dev, M, K, N):
    """cad_op_dense_fwd_bf16 in test_gpu_res_ops.VARIANTS' forms, then the weight gradient"""
    x, w = _z(dev, M, K, bf16=True), _z(dev, N, K, bf16=True)
    add, addld, mask, mean = _z(dev, M, N), _z(dev, M, N + 8), _z(dev, M, N), _z(dev, N)
    for yb, stats in ((0, 0), (1, 0), (0, 1), (1, 1)):
        y = _z(dev, M, N, bf16=bool(yb))
        mv = mean if stats else None
        _ok(lib, lib.cad_op_dense_fwd_bf16(_p(x), K, 0, K, _p(w), K, 0, N, _p(y), N, 0, yb, None, 0, None, _p(mv), _p(mv),
                                           M, _s()))
    y = _z(dev, M, N)
    for a, ld, mk in ((add, 0, None), (addld, N + 8, None), (add, 0, mask)):
        _ok(lib, lib.cad_op_dense_fwd_bf16(_p(x), K, 0, K, _p(w), K, 0, N, _p(y), N, 0, 0, _p(a), ld, _p(mk), None, None, M,
                                           _s()))
    dz, dw = _z(dev, M, N, bf16=True), _z(dev, N, K)
    _ok(lib, lib.cad_op_dense_wgrad_bf16(_p(dz), N, 0, N, _p(x), K, 0, K, _p(dw), K, M, 0, _s()))


def mx8(lib, dev):
    """cad_op_dense_x8 on both tiles and cad_op_conv3x3_x8 on a 128- and a 256-pixel block"""
    M, K = 100, 128
    for N in (64, 128):
        xq, xs, wq, ws = _z(dev, M, K, u8=True), _z(dev, M, K // 32, u8=True), _z(dev, N, K, u8=True), _z(dev, N, K // 32, u8=True)
        _ok(lib, lib.cad_op_dense_x8(_p(xq), _p(xs), K, K, _p(wq), _p(ws), K, N, _p(_z(dev, M, N)), M, _s()))
    B, H, W, cin, ldx, ldw = 1, 4, 64, 64, 128, 640
    for cout in (64, 128):
        xq, xs = _z(dev, B * H * W, ldx, u8=True), _z(dev, B * H * W, ldx // 32, u8=True)
        wq, ws = _z(dev, cout, ldw, u8=True), _z(dev, cout, ldw // 32, u8=True)
        _ok(lib, lib.cad_op_conv3x3_x8(_p(xq), _p(xs), ldx, cin, _p(wq), _p(ws), ldw, cout, _p(_z(dev, B * H * W, cout)), B, H,
                                       W, _s()))


def unet_step(cad, dev):
    """One training step of a 64-feature U-Net at 1 x 128 x 128: the window kernels of every level with the BN
    partials, the bn-sums input gradient (S3), the split store and the big-tile ConvT input gradient (bf16)"""
    B, H, W = 1, 128, 128
    m = cad.BaselineUNet(3, 64, 10.0, batch=B, height=H, width=W)
    m.flat_params.normal_(0.0, 0.05)
    loss = cad.CombinedDepthLoss(batch=B, height=H, width=W)
    tr = cad.Trainer(m, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    K = torch.tensor([[[100.0, 0, 64], [0, 100.0, 64], [0, 0, 1]]], device=dev)
    tr.train_step(torch.rand(B, 3, H, W, device=dev), torch.rand(B, 1, H, W, device=dev) + 1.0, K)


def _cases(cad, dev):
    lib = cad.load_library()
    cases = {}
    for eng in ENGINES:
        for cfg, shape in IM2COL.items():
            cases[f"{eng}/conv3x3 im2col {cfg}"] = (eng, lambda s=shape: conv_f32(lib, dev, *s))
        cases[f"{eng}/conv3x3 act im2col"] = (eng, lambda: conv_act(lib, dev, *IM2COL["C41"]))
        cases[f"{eng}/convT"] = (eng, lambda: convT_f32(lib, dev, 2, 8, 12, 128, 64))
        # split-K: one slab, one-level and two-level reduction (test_gpu_ops.SLAB2's shape)
        cases[f"{eng}/wgrad one slab"] = (eng, lambda: conv_f32(lib, dev, 1, 4, 8, 64, 64, what="wgrad"))
        cases[f"{eng}/wgrad slabs"] = (eng, lambda: conv_f32(lib, dev, 1, 32, 64, 64, 64, what="wgrad"))
        cases[f"{eng}/wgrad two-level slabs"] = (eng, lambda: conv_f32(lib, dev, 1, 100, 256, 64, 64, what="wgrad"))
        if eng != "bf16":   # (the bf16 engine's step runs on the twins: below)
            cases[f"{eng}/unet step"] = (eng, lambda: unet_step(cad, dev))
    for shape in WIN_SHAPES:
        cases[f"s3/conv3x3 window {shape}"] = ("s3", lambda s=shape: conv_f32(lib, dev, *s))
        cases[f"s3/conv3x3 window, no weight twin {shape}"] = ("s3", lambda s=shape: conv_f32(lib, dev, *s), {"CAD_S3_WTWIN": "0"})
    cases["s3/conv3x3 act window"] = ("s3", lambda: conv_act(lib, dev, *WIN_SHAPES[0]))
    for shape in B1_WIN_SHAPES + B1_WIN_MORE:
        cases[f"bf16/conv3x3 twins window {shape}"] = ("bf16", lambda s=shape: conv_ps(lib, dev, *s))
    for cfg, shape in IM2COL_PS.items():
        cases[f"bf16/conv3x3 twins im2col {cfg}"] = ("bf16", lambda s=shape: conv_ps(lib, dev, *s))
    cases["bf16/conv3x3 twins act window"] = ("bf16", lambda: conv_ps_act(lib, dev, *B1_WIN_SHAPES[1]))
    cases["bf16/conv3x3 twins act im2col"] = ("bf16", lambda: conv_ps_act(lib, dev, *IM2COL_PS["C41"]))
    for shape in WGRAD_BF16_SHAPES + [(2, 6, 64, 32, 32, 0)]:
        cases[f"bf16/wgrad twins {shape}"] = ("bf16", lambda s=shape: wgrad_ps(lib, dev, *s))
    for shape in CONVT_BF16_SHAPES:
        cases[f"bf16/convT twins {shape}"] = ("bf16", lambda s=shape: convT_ps(lib, dev, *s))
    cases["bf16/unet step"] = ("bf16", lambda: unet_step(cad, dev))
    for cfg, mkn in {"C22 (DMA)": (200, 72, 136), "C14": (45, 64, 256), "C41": (257, 64, 64), "slabs": (4096, 64, 64)}.items():
        cases[f"bf16/dense {cfg}"] = ("bf16", lambda s=mkn: dense(lib, dev, *s))
    cases["bf16/mx8"] = ("bf16", lambda: mx8(lib, dev))
    return cases


def _names(lib, eng, run, env=None):
    prev = lib.cad_get_gemm_engine()
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    assert lib.cad_set_gemm_engine(ENGINES[eng]) == 0
    torch.cuda.synchronize()
    lib.cad_profile_reset()
    lib.cad_profile_enable(1)
    try:
        run()
        torch.cuda.synchronize()
        n = lib.cad_profile_report(None, 0)
        buf = C.create_string_buffer(n)
        lib.cad_profile_report(buf, n)
    finally:
        lib.cad_profile_enable(0)
        lib.cad_profile_reset()
        lib.cad_set_gemm_engine(prev)
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return sorted(r["name"] for r in json.loads(buf.value.decode()))


def test_profile_names_match_the_golden_file(cad, dev):
    lib = cad.load_library()
    got = {case: _names(lib, *spec) for case, spec in _cases(cad, dev).items()}
    for case, names in got.items():
        assert names, f"{case}: nothing was profiled"
    if RECORD:
        doc = {"_comment": "Kernel names reported by the launch profiler per case of tests/test_gpu_profile_names.py. "
                           "Recorded with CAD_PROFILE_NAMES_RECORD=1 against a build of the commit before the launcher "
                           "refactor (selected through CAD_LIB), never from the code under test.",
               "cases": got}
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    assert sorted(got) == sorted(want), "the case list and the golden file differ: record the file again from the parent build"
    wrong = {case: (sorted(set(got[case]) - set(want[case])), sorted(set(want[case]) - set(got[case])))
             for case in got if got[case] != want[case]}
    assert not wrong, "names differ (new, missing): " + json.dumps(wrong, indent=1)
