"""The S3 window kernels' weight twin (csrc/kernels/gemm_win.hpp WinTwinGeo): the 3 x 3
convolutions' weights are split into their three bf16 planes once per step, in the window kernels' LDS
order, and a stage's B operand is an LDS-DMA copy of that image instead of an fp32 fetch and a split3 in
every workgroup.  The planes are split3's bits and the MFMA order is unchanged, so every result with the
path on (CAD_S3_WTWIN=1) equals the in-loader split's (CAD_S3_WTWIN=0) bit for bit: a wrong tile offset,
stage order, plane or swizzle in the twin, or a stage read before its DMA landed, shows as a difference.
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = os.environ.get("CAD_S3_WTWIN")
        os.environ["CAD_S3_WTWIN"] = self.value

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("CAD_S3_WTWIN", None)
        else:
            os.environ["CAD_S3_WTWIN"] = self.prev


@pytest.fixture
def s3(cad):
    lib = cad.load_library()
    prev = lib.cad_get_gemm_engine()
    assert lib.cad_set_gemm_engine(1) == 0
    yield lib
    lib.cad_set_gemm_engine(prev)


FWD_SHAPES = [  # B, H, W, cin, cout
    (2, 5, 128, 16, 64),    # <2, 128>, BN = 64, one channel block, last block row past H
    (1, 6, 64, 32, 64),     # <4, 64>
    (1, 9, 64, 48, 256),    # <2, 64>: two N tiles, three channel blocks
    (1, 9, 32, 48, 256),    # <4, 32>
    (1, 9, 16, 48, 256),    # <8, 16>
    (1, 9, 8, 48, 256),     # <16, 8>: H < R
]


@pytest.mark.parametrize("B,H,W,cin,cout", FWD_SHAPES)
def test_forward_bit_identical(s3, dev, B, H, W, cin, cout):
    g = torch.Generator().manual_seed(1000 * W + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g).to(dev)
    w = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev)
    out = []
    for sw in ("0", "1"):
        y = torch.full((B, H, W, cout), 7.0, device=dev)
        with _Switch(sw):
            assert s3.cad_op_conv3x3_fwd(_p(x), cin, 0, cin, _p(w), cout, _p(y), cout, 0, B, H, W, _s()) == 0
        torch.cuda.synchronize()
        out.append(y)
    assert out[0].abs().max().item() > 0.1 and not (out[0] == 7).any()
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("cout,cin", [(64, 128), (128, 64)])
def test_dgrad_bit_identical(s3, dev, cout, cin):
    B, H, W = 2, 5, 64   # N = cin: 128 -> <2, 64> (BN = 128), 64 -> <4, 64> (BN = 64), on the repacked weights
    g = torch.Generator().manual_seed(cout * 7 + cin)
    dz = torch.randn(B, H, W, cout, generator=g).to(dev)
    w = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev)
    out = []
    for sw in ("0", "1"):
        dx = torch.full((B, H, W, cin), 7.0, device=dev)
        with _Switch(sw):
            assert s3.cad_op_conv3x3_dgrad(_p(dz), cout, _p(w), cin, _p(dx), cin, B, H, W, _s()) == 0
        torch.cuda.synchronize()
        out.append(dx)
    assert out[0].abs().max().item() > 0.1 and not (out[0] == 7).any()
    assert torch.equal(out[0], out[1])


F, B, H, W = 64, 2, 16, 128


def _train(cad, kind, state, batch, sw):
    with _Switch(sw):
        if kind == "baseline":
            m = cad.BaselineUNet(3, F, 10.0, batch=B, height=H, width=W)
        else:
            m = cad.RayConditionedUNet(3, F, 4, 10.0, batch=B, height=H, width=W)
        m.load_state_dict(state)
        loss = cad.CombinedDepthLoss(1.0, 0.1, 0.001, 0.01, batch=B, height=H, width=W)
        tr = cad.Trainer(m, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
        losses, norms = [], []
        for _ in range(3):
            losses.append(tr.train_step(*batch).clone())
            norms.append(m.last_grad_norm())
        torch.cuda.synchronize()
        return tr.pred.clone(), torch.stack(losses), norms, m.flat_params.clone()


@pytest.mark.parametrize("kind", ["baseline", "rayfilm"])
def test_train_steps_bit_identical(cad, s3, dev, oracle, kind):
    """Three train steps at 16 x 128 (level widths 128 .. 8: all five window shapes at f = 64, the stats
    and BN-sums epilogues, the side-stream backward, the im2col fallback of enc1.conv1)."""
    if kind == "baseline":
        params, bufs = oracle.init_params(F, seed=5), oracle.init_buffers(F)
    else:
        params, bufs = oracle.init_params(F, seed=5, model=kind), oracle.init_buffers(F, model=kind)
    state = dict(params)
    state.update(bufs)
    batch = [torch.from_numpy(a).to(dev) for a in oracle.synth_batch(B, H, W)]
    off = _train(cad, kind, state, batch, "0")
    on = _train(cad, kind, state, batch, "1")
    assert torch.isfinite(off[1]).all() and off[2][0] > 0
    assert torch.equal(on[0], off[0]), "predictions differ"
    assert torch.equal(on[1], off[1]), "loss5 differs"
    assert on[2] == off[2], "gradient norms differ"
    assert torch.equal(on[3], off[3]), "parameters differ"
