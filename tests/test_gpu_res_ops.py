"""Operator-level parity of the config-5 (ResNet-50 U-Net) kernels, one launcher per call through the
cad_op_* entry points: the dense GEMMs on bf16 twins (every tile config, the LDS-DMA kernel's seven
epilogues at M / N / K tails, the register-staged fallbacks), im2col / col2im, MaxPool2d(3, 2, 1), the
bottleneck join and the element-wise / layout passes of csrc/kernels/res_kernels.hip, each against a
plain fp64 (or bit-exact) CPU restatement.

Every buffer is poisoned outside the view under test: input rows wider than the view hold NaN in the
columns outside it and in guard rows after the last, outputs are pre-filled with a sentinel that must
survive in every column outside the view and in guard rows after it.  One pattern for over-reads at
tails and for stray stores.

Tolerances.  fp32 outputs: normalised max error < 2e-5 (test_gpu_ops.TOL: the same arithmetic, fp32
accumulation of exact bf16 products).  bf16 outputs: within one bf16 spacing (floored at that of 2^-10
of the largest output) of the rounded fp64 value, on fewer than 1e-2 of the elements (a condition, not
a measurement: a torch fp32 matmul of the same operands differs from the rounded fp64 result in at most
2.1e-4 of them at these shapes).  BN statistics: mean and 1/invstd^2 - eps against the fp64 mean and
biased variance of the y the kernel returned, within 2e-5 of the fp64 standard deviation / variance (a
tile that counts its padding rows misses by O(1/M)).

Measured on MI355X (recorded, not asserted), LDS-DMA path, worst over the dense-forward cases: fp32
normalised error 6.0e-7 of the 2e-5 budget ((130, 2048, 512)); bf16 differing share 1.5e-4 of the 1e-2
budget (the same shape; 0 at (300, 576, 192), (129, 8, 136), (45, 64, 256)); BN mean 4.4e-7 and
variance 2.1e-6 of their 2e-5.  Dense weight gradient: 8.2e-7 ((136, 72, 3100) in one split)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, max_rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
SENT = -768.0          # exact in bf16 and fp32
NAN = float("nan")
EPS = 1e-5
GUARD = 3              # sentinel rows after every output


@pytest.fixture(autouse=True)
def bf16_engine(cad):
    lib = cad.load_library()
    prev = lib.cad_get_gemm_engine()
    assert lib.cad_set_gemm_engine(2) == 0
    yield lib
    lib.cad_set_gemm_engine(prev)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, st):
    assert st == 0, lib.cad_last_error()


def _refused(lib, st):
    assert st == 1, st            # CAD_ERR_INVALID
    assert lib.cad_last_error(), "no message"


def embed(t, ld, coff, fill=NAN):
    """rows of t (2-D) at columns [coff, coff + width) of rows of ld; `fill` everywhere else and in GUARD
    rows after the last"""
    rows, width = t.shape
    buf = torch.full((rows + GUARD, ld), fill, dtype=t.dtype)
    buf[:rows, coff:coff + width] = t
    return buf


def outbuf(rows, ld, dtype, dev):
    return torch.full((rows + GUARD, ld), SENT, dtype=dtype, device=dev)


def take(buf, rows, coff, width):
    """the view's values (CPU); asserts the sentinel everywhere else"""
    b = buf.cpu()
    keep = torch.ones_like(b, dtype=torch.bool)
    keep[:rows, coff:coff + width] = False
    assert (b[keep] == SENT).all(), "store outside the output view"
    return b[:rows, coff:coff + width].contiguous()


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def bf16_close(got, ref64):
    """test_convT_fwd_bf16's rule; returns the differing share"""
    want = ref64.bfloat16().float()
    got = got.float()
    diff = (got - want).abs()
    big = torch.maximum(got.abs(), want.abs()).clamp_min(2.0 ** -10 * want.abs().max().item())
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
    share = (diff > 0).float().mean().item()
    assert (diff <= ulp).all(), (diff / ulp).max().item()
    assert share < 1e-2, share
    return share


# ------------------------------------------------------------------------------------------------
# dense forward
# ------------------------------------------------------------------------------------------------
DENSE = [  # (M, K, N)
    (200, 72, 136),     # C22 (DMA): M, N, K tails; one partial K stage
    (300, 576, 192),    # C22
    (130, 2048, 512),   # C22
    (129, 8, 136),      # C22: a single, partial K stage
    (45, 64, 256),      # C14: 3 x 3 x 5 rows, the deepest level of 96 x 160 at B = 3
    (600, 200, 64),     # C41: the stem's Kp = 200
    (257, 64, 64),      # C41: narrow-N tile with an M tail
]
VARIANTS = ["f32", "b16", "stats", "stats_b16", "add", "add_ld", "add_mask"]


@functools.lru_cache(maxsize=None)
def dense_case(M, K, N):
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    add = torch.randn(M, N, generator=g)
    mask = torch.randn(M, N, generator=g)
    flat = mask.view(-1)
    flat[0::5] = 0.0
    flat[1::5] = -0.0
    ref = x.double() @ w.double().T
    return x, w, add, mask, ref


def dense_call(lib, dev, M, K, N, *, y, ldy, ycoff, y_bf16=0, add=None, ldadd=0, mask=None, mean=None, invstd=None):
    x, w = dense_case(M, K, N)[:2]
    xg, wg = embed(x, K + 24, 8).to(dev), embed(w, K + 24, 8).to(dev)
    st = lib.cad_op_dense_fwd_bf16(_p(xg), K + 24, 8, K, _p(wg), K + 24, 8, N, _p(y), ldy, ycoff, y_bf16, _p(add), ldadd,
                                   _p(mask), _p(mean), _p(invstd), M, _s())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,K,N", DENSE)
def test_dense_fwd(cad, dev, M, K, N, variant):
    """cad_op_dense_fwd_bf16 (dense_fwd_ps) against x.double() @ w.double().T on the bf16 values; operands
    read through views (ld = K + 24, coff = 8, NaN outside)."""
    lib = cad.load_library()
    x, w, add, mask, ref = dense_case(M, K, N)
    ldy, yc = N + 16, 8
    b16 = variant in ("b16", "stats_b16")
    stats = variant in ("stats", "stats_b16")
    if variant in ("f32", "b16", "stats", "stats_b16"):
        y = outbuf(M, ldy, torch.bfloat16 if b16 else torch.float32, dev)
        mean = torch.full((N + 4,), SENT, device=dev) if stats else None
        invstd = torch.full((N + 4,), SENT, device=dev) if stats else None
        _ok(lib, dense_call(lib, dev, M, K, N, y=y, ldy=ldy, ycoff=yc, y_bf16=int(b16), mean=mean, invstd=invstd))
        got = take(y, M, yc, N)
        if b16:
            print(f"RESOPS dense {variant} {(M, K, N)} bf16 differing share {bf16_close(got, ref):.3e}")
        else:
            err = max_rel_err(got, ref)
            print(f"RESOPS dense {variant} {(M, K, N)} fp32 err {err:.3e}")
            assert err < TOL
        if stats:
            assert (mean[N:] == SENT).all() and (invstd[N:] == SENT).all()
            yd = got.double()
            mu, var = yd.mean(0), yd.var(0, unbiased=False)
            e_mu = ((mean[:N].cpu().double() - mu).abs() / var.sqrt()).max().item()
            got_var = 1.0 / invstd[:N].cpu().double() ** 2 - float(torch.tensor(EPS, dtype=torch.float32))
            e_var = ((got_var - var).abs() / var).max().item()
            print(f"RESOPS dense {variant} {(M, K, N)} mean err {e_mu:.3e} var err {e_var:.3e}")
            assert e_mu < 2e-5 and e_var < 2e-5, (e_mu, e_var)
        return
    if variant == "add":      # add rows as y's: a separate buffer, then in place (add == y)
        want = ref + add.double()
        y = outbuf(M, ldy, torch.float32, dev)
        addg = embed(add, ldy, yc).to(dev)
        _ok(lib, dense_call(lib, dev, M, K, N, y=y, ldy=ldy, ycoff=yc, add=addg))
        err = max_rel_err(take(y, M, yc, N), want)
        print(f"RESOPS dense add {(M, K, N)} fp32 err {err:.3e}")
        assert err < TOL
        y = outbuf(M, ldy, torch.float32, dev)
        y[:M, yc:yc + N] = add.to(dev)
        _ok(lib, dense_call(lib, dev, M, K, N, y=y, ldy=ldy, ycoff=yc, add=y))
        err = max_rel_err(take(y, M, yc, N), want)
        print(f"RESOPS dense add-in-place {(M, K, N)} fp32 err {err:.3e}")
        assert err < TOL
    elif variant == "add_ld":   # add rows of their own stride
        ldadd = N + 8
        y = outbuf(M, ldy, torch.float32, dev)
        addg = embed(add, ldadd, 0).to(dev)
        _ok(lib, dense_call(lib, dev, M, K, N, y=y, ldy=ldy, ycoff=0, add=addg, ldadd=ldadd))
        err = max_rel_err(take(y, M, 0, N), ref + add.double())
        print(f"RESOPS dense add_ld {(M, K, N)} fp32 err {err:.3e}")
        assert err < TOL
    else:                       # add, then zero where the mask is not > 0 (zero, -0.0, negatives)
        y = outbuf(M, ldy, torch.float32, dev)
        addg, maskg = embed(add, ldy, yc).to(dev), embed(mask, ldy, yc).to(dev)
        _ok(lib, dense_call(lib, dev, M, K, N, y=y, ldy=ldy, ycoff=yc, add=addg, mask=maskg))
        got = take(y, M, yc, N)
        keep = mask > 0
        assert 0.2 < keep.float().mean().item() < 0.4
        assert same_bits(got[~keep], torch.zeros_like(got[~keep]))
        err = max_rel_err(got, torch.where(keep, ref + add.double(), torch.zeros_like(ref)))
        print(f"RESOPS dense add_mask {(M, K, N)} fp32 err {err:.3e}")
        assert err < TOL


def test_dense_fwd_refusals(cad, dev):
    """Argument combinations the launcher does not take return CAD_ERR_INVALID with a message and launch
    nothing."""
    lib = cad.load_library()
    M, K, N = DENSE[0]
    _, _, add, mask, _ = dense_case(M, K, N)
    ldy = N + 16
    addg, maskg = embed(add, ldy, 8).to(dev), embed(mask, ldy, 8).to(dev)
    mean, invstd = torch.zeros(N, device=dev), torch.zeros(N, device=dev)

    def refused(**kw):
        b16 = kw.get("y_bf16", 0)
        y = outbuf(M, ldy, torch.bfloat16 if b16 else torch.float32, dev)
        _refused(lib, dense_call(lib, dev, M, K, N, y=y, ldy=ldy, **kw))
        assert (y == SENT).all()
    refused(ycoff=8, mask=maskg)                                       # a mask without add
    refused(ycoff=0, add=addg, ldadd=N + 8, mask=maskg)                # own-stride add with a mask
    refused(ycoff=8, add=addg, ldadd=N + 8)                            # own-stride add with ycoff
    refused(ycoff=8, add=addg, mean=mean, invstd=invstd)               # add with stats
    refused(ycoff=8, add=addg, y_bf16=1)                               # add with bf16 output


def test_register_staged_c22_in_child(dev):
    """CAD_DENSEDMA=0 (read once per process): the dense-forward cases above on the register-staged C22
    kernels and the add / mask passes, in a fresh interpreter."""
    if os.environ.get("CAD_RES_OPS_CHILD"):
        pytest.skip("the outer case of the CAD_DENSEDMA=0 run")
    env = dict(os.environ, CAD_DENSEDMA="0", CAD_RES_OPS_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_dense_fwd"], cwd=ROOT, env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert f"{len(DENSE) * len(VARIANTS) + 1} passed" in r.stdout, r.stdout[-2000:]


# ------------------------------------------------------------------------------------------------
# dense weight gradient
# ------------------------------------------------------------------------------------------------
WGRAD = [  # (N, K, M, view): view = operands at coff 8 of rows 24 wider
    (136, 72, 300, True), (64, 200, 600, True), (256, 64, 45, False), (512, 2048, 130, False),
    (136, 72, 3100, True),   # 97 K stages of 32 rows: three split-K slabs with the full slab
]


def _profile(lib):
    import json
    n = lib.cad_profile_report(None, 0)
    buf = C.create_string_buffer(n)
    lib.cad_profile_report(buf, n)
    return json.loads(buf.value.decode())


@pytest.mark.parametrize("N,K,M,view", WGRAD)
def test_dense_wgrad(cad, dev, N, K, M, view):
    """cad_op_dense_wgrad_bf16 (dense_wgrad_ps): dw[n][k] = sum_m dz[m][n] x[m][k] against fp64, with the
    launcher's own slab and with the slab capped to one split; the launch profile shows which ran."""
    lib = cad.load_library()
    g = torch.Generator().manual_seed(N + K + M)
    dz = torch.randn(M, N, generator=g).bfloat16()
    x = torch.randn(M, K, generator=g).bfloat16()
    ref = dz.double().T @ x.double()
    pad, co = (24, 8) if view else (0, 0)
    dzg, xg = embed(dz, N + pad, co).to(dev), embed(x, K + pad, co).to(dev)
    for slab_max in (0, 1):
        dw = outbuf(N, K, torch.float32, dev)
        torch.cuda.synchronize()
        lib.cad_profile_reset()
        lib.cad_profile_enable(1)
        try:
            st = lib.cad_op_dense_wgrad_bf16(_p(dzg), N + pad, co, N, _p(xg), K + pad, co, K, _p(dw), K, M, slab_max, _s())
            torch.cuda.synchronize()
            prof = _profile(lib)
        finally:
            lib.cad_profile_enable(0)
        _ok(lib, st)
        reduces = sum(r["launches"] for r in prof if "k_slab_reduce" in r["name"])
        assert reduces == (1 if M >= 2048 and slab_max == 0 else 0), prof
        err = max_rel_err(take(dw, N, 0, K), ref)
        print(f"RESOPS wgrad {(N, K, M)} slab_max {slab_max} err {err:.3e}")
        assert err < TOL
    dw = outbuf(N, K + 8, torch.float32, dev)
    _refused(lib, lib.cad_op_dense_wgrad_bf16(_p(dzg), N + pad, co, N, _p(xg), K + pad, co, K, _p(dw), K + 8, M, 0, _s()))
    torch.cuda.synchronize()
    assert (dw == SENT).all()


# ------------------------------------------------------------------------------------------------
# im2col / col2im
# ------------------------------------------------------------------------------------------------
def out_hw(H, W, KH, KW, S, P):
    return (H + 2 * P - KH) // S + 1, (W + 2 * P - KW) // S + 1


def im2col_ref(x, KH, KW, S, P, Kp):
    """x (B, H, W, C) -> (B Ho Wo, Kp): k = (ky KW + kx) C + c, zero outside the image and in the pad columns"""
    B, H, W, Cc = x.shape
    Ho, Wo = out_hw(H, W, KH, KW, S, P)
    xp = F.pad(x, (0, 0, P, P, P, P))
    taps = [xp[:, ky:ky + S * (Ho - 1) + 1:S, kx:kx + S * (Wo - 1) + 1:S, :] for ky in range(KH) for kx in range(KW)]
    col = torch.cat(taps, -1).reshape(B * Ho * Wo, KH * KW * Cc)
    return F.pad(col, (0, Kp - KH * KW * Cc))


IM2COL = [  # C, KH, S, P, Kp, (B, H, W), ldx, xcoff, twin
    (4, 7, 2, 3, 200, (2, 14, 18), 4, 0, False),      # the stem (k_im2col_c4)
    (4, 7, 2, 3, 200, (2, 14, 18), 12, 4, False),     # ... through a view
    (12, 3, 1, 1, 112, (2, 5, 7), 20, 4, False),      # 8-wide groups straddle taps
    (16, 3, 2, 1, 152, (2, 7, 9), 16, 0, False),
    (16, 3, 2, 1, 152, (2, 7, 9), 32, 8, True),
    (64, 3, 2, 1, 576, (2, 7, 9), 64, 0, False),
    (64, 3, 2, 1, 576, (2, 7, 9), 80, 8, True),
    (8, 1, 2, 0, 8, (2, 7, 9), 8, 0, False),          # 1x1 stride 2
    (8, 1, 2, 0, 8, (2, 7, 9), 24, 8, True),
]


@pytest.mark.parametrize("Cc,Kk,S,P,Kp,shape,ldx,xcoff,twin", IM2COL)
def test_im2col(cad, dev, Cc, Kk, S, P, Kp, shape, ldx, xcoff, twin):
    """cad_op_im2col (im2col_f32 / im2col_ps) bit-exact against a CPU gather (+ .bfloat16() for fp32)."""
    lib = cad.load_library()
    B, H, W = shape
    g = torch.Generator().manual_seed(Cc * 100 + Kk + ldx)
    x = torch.randn(B, H, W, Cc, generator=g)
    if twin:
        x = x.bfloat16()
    want = im2col_ref(x, Kk, Kk, S, P, Kp).bfloat16()
    xg = embed(x.reshape(-1, Cc), ldx, xcoff).to(dev)
    rows = want.shape[0]
    col = outbuf(rows, Kp, torch.bfloat16, dev)
    _ok(lib, lib.cad_op_im2col(_p(xg), int(twin), ldx, xcoff, Cc, B, H, W, Kk, Kk, S, P, _p(col), Kp, _s()))
    torch.cuda.synchronize()
    assert same_bits(take(col, rows, 0, Kp), want)


COL2IM = [  # C, KH, S, P, Kc, (B, H, W), lddx
    (8, 3, 2, 1, 72, (2, 7, 9), 16),
    (4, 7, 2, 3, 200, (2, 14, 18), 4),      # the stem: pad columns [196, 200) hold NaN
    (16, 3, 1, 1, 144, (1, 5, 6), 16),
]


@pytest.mark.parametrize("Cc,Kk,S,P,Kc,shape,lddx", COL2IM)
def test_col2im(cad, dev, Cc, Kk, S, P, Kc, shape, lddx):
    """cad_op_col2im against the fp64 adjoint (F.fold with the k axis in torch's order), and the pairing
    <col2im(d), x> = <d, im2col(x)> with the kernel's own im2col on bf16-exact data."""
    lib = cad.load_library()
    B, H, W = shape
    Ho, Wo = out_hw(H, W, Kk, Kk, S, P)
    taps, L = Kk * Kk, Ho * Wo
    g = torch.Generator().manual_seed(Cc + Kk + Kc)
    d = torch.randn(B * L, taps * Cc, generator=g).bfloat16().float()
    x = torch.randn(B, H, W, Cc, generator=g).bfloat16().float()
    # fold wants (B, C * taps, L) with the channel index c * taps + tap
    dd = d.double().reshape(B, L, taps, Cc).permute(0, 3, 2, 1).reshape(B, Cc * taps, L)
    ref = F.fold(dd, (H, W), (Kk, Kk), padding=P, stride=S).permute(0, 2, 3, 1).reshape(B * H * W, Cc)
    dg = embed(d, Kc, 0).to(dev)
    dx = outbuf(B * H * W, lddx, torch.float32, dev)
    _ok(lib, lib.cad_op_col2im(_p(dg), Kc, Cc, B, H, W, Kk, Kk, S, P, _p(dx), lddx, _s()))
    torch.cuda.synchronize()
    got = take(dx, B * H * W, 0, Cc)
    assert max_rel_err(got, ref) < TOL
    # the two layouts agree: the kernel's im2col of x, paired with d
    Kp = (taps * Cc + 7) // 8 * 8
    col = outbuf(B * L, Kp, torch.bfloat16, dev)
    xg = x.reshape(-1, Cc).contiguous().to(dev)
    _ok(lib, lib.cad_op_im2col(_p(xg), 0, Cc, 0, Cc, B, H, W, Kk, Kk, S, P, _p(col), Kp, _s()))
    torch.cuda.synchronize()
    colx = take(col, B * L, 0, Kp)[:, :taps * Cc].double()
    lhs = (got.double() * x.reshape(-1, Cc).double()).sum().item()
    rhs = (d.double() * colx).sum().item()
    # col2im sums at most `taps` fp32 terms per element: (taps - 1) roundings of the partial sums
    bound = taps * 2.0 ** -24 * (d.abs().double() * colx.abs()).sum().item()
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ------------------------------------------------------------------------------------------------
# MaxPool2d(3, 2, 1)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [8, 64])
@pytest.mark.parametrize("B,H,W", [(2, 9, 11), (1, 8, 8)])
def test_maxpool3s2(cad, dev, B, H, W, Cc):
    """Forward bit-exact against F.max_pool2d(x, 3, 2, 1) with its indices (ties: first in scan order, also
    across a window's rows and on the padded border; one NaN), the twin, and the gather backward against
    fp64 autograd, alone and with an added matrix."""
    lib = cad.load_library()
    g = torch.Generator().manual_seed(B * H * W + Cc)
    x = torch.randn(B, H, W, Cc, generator=g)
    x[..., 0] = 1.5                                                   # every window a full tie
    x[..., 1:4] = torch.randint(-2, 3, (B, H, W, 3), generator=g).float()   # ties everywhere
    x[0, 1, :, 4] = 3.0                                               # a tie along a row ...
    x[0, 2, :, 4] = 3.0                                               # ... and across the window's rows
    x[0, 0, :, 5] = 4.0                                               # on the padded border
    x[0, :, 0, 5] = 4.0
    x[0, 2, 3, 6] = NAN
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xn = x.permute(0, 3, 1, 2).contiguous()
    ref, ridx = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    rows = B * Ho * Wo
    xg = x.to(dev)
    out = outbuf(rows, Cc, torch.float32, dev)
    twin = outbuf(rows, Cc, torch.bfloat16, dev)
    idx = torch.full((rows + GUARD, Cc), 99, dtype=torch.uint8, device=dev)
    _ok(lib, lib.cad_op_maxpool3s2_fwd(_p(xg), Cc, B, H, W, _p(out), _p(idx), _p(twin), _s()))
    torch.cuda.synchronize()
    got = take(out, rows, 0, Cc)
    want = ref.permute(0, 2, 3, 1).reshape(rows, Cc)
    assert torch.equal(got.isnan(), want.isnan()) and want.isnan().sum() >= 1
    assert same_bits(got.nan_to_num(nan=0.0), want.nan_to_num(nan=0.0))
    # the twin: bitwise out.bfloat16(); at the NaN both are NaN (the payload of a converted NaN is the
    # converter's own: the hardware conversion writes 0x7FC0, torch's 0xFFFF)
    tw, tw_want = take(twin, rows, 0, Cc), got.bfloat16()
    assert torch.equal(tw.isnan(), got.isnan())
    assert same_bits(tw.nan_to_num(nan=0.0), tw_want.nan_to_num(nan=0.0))
    assert (idx[rows:] == 99).all()
    k = idx[:rows].cpu().long().reshape(B, Ho, Wo, Cc).permute(0, 3, 1, 2)
    oy = torch.arange(Ho).view(1, 1, -1, 1)
    ox = torch.arange(Wo).view(1, 1, 1, -1)
    assert torch.equal((2 * oy - 1 + k // 3) * W + 2 * ox - 1 + k % 3, ridx)
    # two windows that select the same pixel both deliver their gradient
    flat = (ridx + (torch.arange(B * Cc).view(B, Cc, 1, 1) * H * W)).flatten()
    assert torch.bincount(flat).max().item() >= 2
    # out-only and twin-only calls write the same
    out2 = outbuf(rows, Cc, torch.float32, dev)
    _ok(lib, lib.cad_op_maxpool3s2_fwd(_p(xg), Cc, B, H, W, _p(out2), _p(idx), None, _s()))
    torch.cuda.synchronize()
    assert same_bits(take(out2, rows, 0, Cc).nan_to_num(nan=0.0), got.nan_to_num(nan=0.0))
    # backward through the kernel's own codes
    dout = torch.randn(B, Ho, Wo, Cc, generator=g)
    xd = xn.double().requires_grad_()
    F.max_pool2d(xd, 3, 2, 1).backward(dout.permute(0, 3, 1, 2).double())
    gref = xd.grad.permute(0, 2, 3, 1).reshape(B * H * W, Cc)
    doutg = dout.to(dev)
    dx = outbuf(B * H * W, Cc, torch.float32, dev)
    _ok(lib, lib.cad_op_maxpool3s2_bwd(_p(doutg), _p(idx), Cc, B, H, W, _p(dx), None, 0, _s()))
    torch.cuda.synchronize()
    assert max_rel_err(take(dx, B * H * W, 0, Cc), gref) < TOL
    add = torch.randn(B * H * W, Cc, generator=g)
    addg = embed(add, Cc + 8, 0).to(dev)
    dx = outbuf(B * H * W, Cc, torch.float32, dev)
    _ok(lib, lib.cad_op_maxpool3s2_bwd(_p(doutg), _p(idx), Cc, B, H, W, _p(dx), _p(addg), Cc + 8, _s()))
    torch.cuda.synchronize()
    assert max_rel_err(take(dx, B * H * W, 0, Cc), gref + add.double()) < TOL


# ------------------------------------------------------------------------------------------------
# bottleneck join
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_bf16", [0, 1])
@pytest.mark.parametrize("proj", [0, 1])
@pytest.mark.parametrize("Cc", [32, 96])
def test_bn_add_relu(cad, dev, Cc, proj, y_bf16):
    """out = relu(y s + t + r), r = x (identity, ldx > C) or yd sd + td (projection), elementwise against
    fp64 within 6 fp32 roundings of the terms' magnitudes (contracted or not; the same absolute bound
    covers the elements at the ReLU corner); the twin is the kernel's own output rounded, the MX-fp8 copy
    what cad_op_mx8_quantize writes from that twin."""
    lib = cad.load_library()
    M = 37
    g = torch.Generator().manual_seed(Cc + 2 * proj + y_bf16)
    ydt = torch.bfloat16 if y_bf16 else torch.float32
    y = torch.randn(M, Cc, generator=g).to(ydt)
    s, t = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    sd, td = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    main = y.float() * s + t
    corner = torch.rand(M, Cc, generator=g) < 0.2          # the sum lands within rounding of the ReLU corner
    if proj:
        yd = torch.where(corner, -(main + td) / sd, torch.randn(M, Cc, generator=g)).to(ydt)
        r64 = yd.double() * sd.double() + td.double()
        mag = (yd.double() * sd.double()).abs() + td.double().abs()
        xg, ydg, ldx = None, yd.to(dev), 0
    else:
        x = torch.where(corner, -main, torch.randn(M, Cc, generator=g))
        r64, mag = x.double(), x.double().abs()
        ldx = Cc + 8
        xg, ydg = embed(x, ldx, 0).to(dev), None
    pre = y.double() * s.double() + t.double() + r64
    ref = pre.clamp_min(0.0)
    bound = 6 * 2.0 ** -24 * ((y.double() * s.double()).abs() + t.double().abs() + mag)
    if not (proj and y_bf16):   # (a bf16 yd cannot cancel the main branch to within fp32 rounding)
        assert ((pre.abs() <= bound) & corner).sum() > 0
    yg, sg, tg, sdg, tdg = y.to(dev), s.to(dev), t.to(dev), sd.to(dev), td.to(dev)
    ldq = 128
    out = outbuf(M, Cc, torch.float32, dev)
    twin = outbuf(M, Cc, torch.bfloat16, dev)
    q = torch.full((M + GUARD, ldq), 0x5A, dtype=torch.uint8, device=dev)
    qs = torch.full((M + GUARD, ldq // 32), 0x5A, dtype=torch.uint8, device=dev)
    args = (_p(yg), y_bf16, _p(sg), _p(tg), _p(ydg), _p(sdg) if proj else None, _p(tdg) if proj else None, _p(xg), ldx,
            Cc, M)
    _ok(lib, lib.cad_op_bn_add_relu(*args, _p(out), _p(twin), _p(q), _p(qs), ldq, _s()))
    torch.cuda.synchronize()
    got = take(out, M, 0, Cc)
    excess = ((got.double() - ref).abs() - bound).max().item()
    assert excess <= 0, excess
    tw = take(twin, M, 0, Cc)
    assert same_bits(tw, got.bfloat16())
    q2, qs2 = torch.full_like(q, 0x5A), torch.full_like(qs, 0x5A)
    twg = tw.to(dev)
    _ok(lib, lib.cad_op_mx8_quantize(_p(twg), 1, Cc, 0, Cc, M, _p(q2), _p(qs2), ldq, 0, _s()))
    torch.cuda.synchronize()
    assert torch.equal(q, q2) and torch.equal(qs, qs2)
    assert not (q[:M, :Cc] == 0x5A).all()
    # without the twin and the MX copy: the same fp32 output
    out2 = outbuf(M, Cc, torch.float32, dev)
    _ok(lib, lib.cad_op_bn_add_relu(*args, _p(out2), None, None, None, 0, _s()))
    torch.cuda.synchronize()
    assert same_bits(take(out2, M, 0, Cc), got)


def test_bn_add_relu_refuses_mx_copy_of_partial_blocks(cad, dev):
    lib = cad.load_library()
    M, Cc = 5, 40
    y, v, x = torch.zeros(M, Cc, device=dev), torch.ones(Cc, device=dev), torch.zeros(M, Cc, device=dev)
    out = outbuf(M, Cc, torch.float32, dev)
    q = torch.zeros(M, 128, dtype=torch.uint8, device=dev)
    qs = torch.zeros(M, 4, dtype=torch.uint8, device=dev)
    _refused(lib, lib.cad_op_bn_add_relu(_p(y), 0, _p(v), _p(v), None, None, None, _p(x), Cc, Cc, M, _p(out), None, _p(q),
                                         _p(qs), 128, _s()))
    torch.cuda.synchronize()
    assert (out == SENT).all()
    _ok(lib, lib.cad_op_bn_add_relu(_p(y), 0, _p(v), _p(v), None, None, None, _p(x), Cc, Cc, M, _p(out), None, None, None,
                                    0, _s()))
    torch.cuda.synchronize()
    assert (take(out, M, 0, Cc) == 1).all()


# ------------------------------------------------------------------------------------------------
# element-wise and layout kernels
# ------------------------------------------------------------------------------------------------
def mask_values(shape, g):
    m = torch.randn(shape, generator=g)
    flat = m.view(-1)
    flat[0::4] = 0.0
    flat[1::4] = -0.0
    return m


def test_relu_mask_and_mask_inplace(cad, dev):
    lib = cad.load_library()
    M, Cc = 37, 24
    g = torch.Generator().manual_seed(5)
    gr, out = torch.randn(M, Cc, generator=g), mask_values((M, Cc), g)
    ldg, gcoff = Cc + 12, 4
    gg, og = embed(gr, ldg, gcoff).to(dev), out.to(dev)
    gs = outbuf(M, Cc, torch.float32, dev)
    _ok(lib, lib.cad_op_relu_mask(_p(gg), ldg, gcoff, _p(og), Cc, M, _p(gs), _s()))
    torch.cuda.synchronize()
    assert same_bits(take(gs, M, 0, Cc), torch.where(out > 0, gr, torch.zeros_like(gr)))
    ldy, ycoff = Cc + 16, 8
    y = outbuf(M, ldy, torch.float32, dev)
    y[:M, ycoff:ycoff + Cc] = gr.to(dev)
    mg = embed(out, ldy, ycoff).to(dev)
    _ok(lib, lib.cad_op_mask_inplace(_p(y), ldy, ycoff, _p(mg), Cc, M, _s()))
    torch.cuda.synchronize()
    assert same_bits(take(y, M, ycoff, Cc), torch.where(out > 0, gr, torch.zeros_like(gr)))


@pytest.mark.parametrize("S,shape", [(1, (2, 4, 5)), (2, (2, 7, 9))])
def test_add_strided_and_copy_twin(cad, dev, S, shape):
    lib = cad.load_library()
    B, H, W = shape
    Ho, Wo = (H - 1) // S + 1, (W - 1) // S + 1
    Cc = 16
    g = torch.Generator().manual_seed(S)
    # dst[(b, S oy, S ox)][c] += src[(b, oy, ox)][scoff + c]: one fp32 add
    dst0 = torch.randn(B, H, W, Cc, generator=g)
    src = torch.randn(B, Ho, Wo, Cc, generator=g)
    want = dst0.clone()
    want[:, ::S, ::S] += src
    lddst, ldsrc, scoff = Cc + 4, Cc + 12, 4
    dst = outbuf(B * H * W, lddst, torch.float32, dev)
    dst[:B * H * W, :Cc] = dst0.reshape(-1, Cc).to(dev)
    srcg = embed(src.reshape(-1, Cc), ldsrc, scoff).to(dev)
    _ok(lib, lib.cad_op_add_strided(_p(dst), lddst, _p(srcg), ldsrc, scoff, Cc, B, H, W, S, _s()))
    torch.cuda.synchronize()
    assert same_bits(take(dst, B * H * W, 0, Cc), want.reshape(-1, Cc))
    # twin rows dst[(b, oy, ox)][dcoff + c] = src[(b, S oy, S ox)][coff + c]
    t = torch.randn(B, H, W, Cc, generator=g).bfloat16()
    lds, coff, ldd, dcoff = Cc + 16, 8, Cc + 24, 8
    tg = embed(t.reshape(-1, Cc), lds, coff).to(dev)
    d = outbuf(B * Ho * Wo, ldd, torch.bfloat16, dev)
    _ok(lib, lib.cad_op_copy_twin(_p(tg), lds, coff, Cc, B, H, W, S, _p(d), ldd, dcoff, _s()))
    torch.cuda.synchronize()
    assert same_bits(take(d, B * Ho * Wo, dcoff, Cc), t[:, ::S, ::S].reshape(-1, Cc))


@pytest.mark.parametrize("N,K", [(40, 72), (33, 31), (64, 200)])
def test_transpose_split(cad, dev, N, K):
    """wt[k][n] = bf16(w[n][k]), round-to-nearest-even (ties both ways), through ldw > K."""
    lib = cad.load_library()
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g)
    w[0, :4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20])
    w[N - 1, K - 1] = 1 + 3 * 2.0 ** -8
    ldw = K + 5
    wg = embed(w, ldw, 0).to(dev)
    wt = outbuf(K, N, torch.bfloat16, dev)
    _ok(lib, lib.cad_op_transpose_split(_p(wg), ldw, N, K, _p(wt), _s()))
    torch.cuda.synchronize()
    want = w.T.contiguous().bfloat16()
    assert want[0, 0].item() == 1.0 and want[1, 0].item() == 1 + 2.0 ** -6
    assert same_bits(take(wt, K, 0, N), want)


# ------------------------------------------------------------------------------------------------
# aliasing guard
# ------------------------------------------------------------------------------------------------
def test_alias_guard_on_res_launchers(cad, dev):
    """With the launch-level aliasing guard on, an output over an input is refused (CAD_ERR_INVALID,
    nothing launched) by col2im, copy_twin and maxpool3s2_bwd; the declared in-place uses run: add == y
    in the dense forward, relu_mask writing over g."""
    lib = cad.load_library()
    prev = lib.cad_set_alias_check(1)
    try:
        def refused(st, buf, before):
            msg = lib.cad_last_error().decode()
            torch.cuda.synchronize()
            assert st == 1 and "alias" in msg, (st, msg)
            assert same_bits(buf.cpu(), before)
        B, H, W, Cc = 1, 5, 6, 16
        d = torch.randn(B * H * W, 9 * Cc, device=dev)
        refused(lib.cad_op_col2im(_p(d), 9 * Cc, Cc, B, H, W, 3, 3, 1, 1, _p(d), 9 * Cc, _s()), d, d.cpu())
        t = torch.randn(B * H * W, Cc, device=dev).bfloat16()
        refused(lib.cad_op_copy_twin(_p(t), Cc, 0, Cc, B, H, W, 1, _p(t), Cc, 0, _s()), t, t.cpu())
        big = torch.randn(B * H * W, Cc, device=dev)
        idx = torch.zeros(B * 3 * 3, Cc, dtype=torch.uint8, device=dev)
        refused(lib.cad_op_maxpool3s2_bwd(_p(big), _p(idx), Cc, B, H, W, _p(big), None, 0, _s()), big, big.cpu())
        # declared in-place uses
        M, K, N = DENSE[0]
        _, _, add, _, ref = dense_case(M, K, N)
        y = add.to(dev)
        _ok(lib, dense_call(lib, dev, M, K, N, y=y, ldy=N, ycoff=0, add=y))
        assert max_rel_err(y.cpu(), ref + add.double()) < TOL
        gr, out = torch.randn(M, N), torch.randn(M, N)
        gg, og = gr.to(dev), out.to(dev)
        _ok(lib, lib.cad_op_relu_mask(_p(gg), N, 0, _p(og), N, M, _p(gg), _s()))
        torch.cuda.synchronize()
        assert same_bits(gg.cpu(), torch.where(out > 0, gr, torch.zeros_like(gr)))
    finally:
        lib.cad_set_alias_check(prev)
