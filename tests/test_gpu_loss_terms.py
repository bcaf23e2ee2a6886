"""The fused depth loss (csrc/kernels/loss_kernels.hip) term by term against the oracle restatement in
float64 on the host (oracle.cad_oracle si_loss / grad_loss / smooth_loss / reproj_loss / loss_and_dpred).

test_gpu_loss.py checks the recipe's weighted sum, where the smoothness (0.001) and reprojection (0.01)
gradients vanish next to the scale-invariant one.  Here every term runs alone (one-hot weights) and in a
mixed sum, at shapes chosen for the edges of pass B's wave walk and of the pyramid kernel.

Tolerance.  Every case also evaluates the restatement in float32 on the host; E32 is its normalised max
error against float64.  E32 < 1e-4 is asserted first (no sgn() argument sits close enough to 0 for fp32
to flip it; no pixel is left out anywhere in this file), then the kernel's normalised max error against
float64 must be <= max(8 E32, 1e-5): 8 for hardware logf / expf / division against libm and another
valid fp32 evaluation order, the floor for cases where E32 is a few ulps by luck.  The five loss values
keep the project's 1e-4 relative bound.

Worst measured on MI355X over every case of this file, kernel error / worst E32 of the term (also in
DESIGN.md next to the loss fixtures): SI 1.22e-7 / 9.98e-8, gradient matching 1.45e-7 / 1.13e-7,
smoothness 2.09e-7 / 2.56e-7, reprojection 2.55e-5 / 2.54e-5 (2 x 33 x 129; the float32 restatement is as
far from float64 as the kernel), mixed 3.98e-7 / 3.99e-7; linearity 4.96e-8.  No floor was widened.
"""
import numpy as np
import pytest
import torch

from conftest import max_rel_err

pytestmark = pytest.mark.gpu

E = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
MIXED = (0.3, 0.7, 1.3, 0.9)
WEIGHTS = {"si": E[0], "grad": E[1], "smooth": E[2], "reproj": E[3], "mixed": MIXED}
EPS32 = float(np.float32(1e-6))   # the kernel's clamp bound as fp32 holds it

# B, H, W: what the shape reaches
SHAPES = [
    (1, 16, 16),    # smallest legal pyramid (scale 3 is 2 x 2), one partly filled wave
    (2, 17, 65),    # odd H, second column group with one lane, scalar pyramid path, trimmed row / column
    (2, 24, 68),    # W % 4 == 0, W % 8 != 0: vector pyramid path with a scalar last block
    (2, 64, 64),    # one exact wave width, lane 63 at the image border
    (1, 16, 128),   # lanes 63 and 0 meet at an interior group boundary
    (2, 33, 129),   # three column groups, the last with one lane; bands of 2 rows with a 1-row tail
    (1, 19, 200),   # last group 8 lanes wide; empty bands
    (5, 50, 70),    # odd B, alternating K, the existing fixture's map size
]


def _pred(B, H, W, seed=0xBEEF):
    from oracle.cad_oracle import u01
    return (np.float32(0.05) + np.float32(9.9) * u01(seed, np.arange(B * H * W, dtype=np.uint64))).reshape(B, 1, H, W)


_INPUTS = {}


def _inputs(B, H, W):
    """(pred, gt, rgb, K) as test_gpu_loss.py makes them; made once per shape and never written to."""
    if (B, H, W) not in _INPUTS:
        from oracle.cad_oracle import synth_batch
        rgb, gt, K = synth_batch(B, H, W)
        _INPUTS[(B, H, W)] = (_pred(B, H, W), gt, rgb, K)
    return _INPUTS[(B, H, W)]


def _restate(pred, gt, rgb, K, w, mask=None, dtype=torch.float64, eps=None):
    """The oracle restatement in `dtype` on the host: ([total, si, grad, smooth, reproj], dL/dpred)."""
    from oracle import cad_oracle as O
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    p, g, im, k = c(pred), c(gt), c(rgb), c(K)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).bool()
    if eps is None:
        total, comps, d = O.loss_and_dpred(p, g, im, k, w, m)
        return [total, comps["si_loss"], comps["grad_loss"], comps["smooth_loss"], comps["reproj_loss"]], d.double()
    p.requires_grad_(True)
    t = [O.si_loss(p, g, eps=eps, valid_mask=m), O.grad_loss(p, g, eps=eps), O.smooth_loss(p, im, eps=eps),
         O.reproj_loss(p, g, k, eps=eps, valid_mask=m)]
    wf = [float(np.float32(x)) for x in w]
    total = sum(a * b for a, b in zip(wf, t))
    total.sum().backward()
    return [float(total.detach().sum())] + [float(x.detach().sum()) for x in t], p.grad.detach().double()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _gpu(cad, dev, w, pred, gt, rgb, K, mask=None, max_batch=None, loss=None):
    """One call on a fresh handle (or `loss`): (loss5 as float64 numpy, dpred on the host)."""
    B, _, H, W = pred.shape
    if loss is None:
        loss = cad.CombinedDepthLoss(*w, batch=max_batch or B, height=H, width=W)
    m = None if mask is None else _t(mask, dev)
    l5, d = loss.forward_with_intrinsics(_t(pred, dev), _t(gt, dev), _t(rgb, dev), _t(K, dev), valid_mask=m)
    return l5.cpu().double().numpy(), d.cpu()


def _bound(tag, d, want, d32):
    """E32 < 1e-4, then max_rel_err(d, want) <= max(8 E32, 1e-5); both figures are printed first."""
    e32 = max_rel_err(d32, want)
    err = max_rel_err(d, want)
    print(f"LOSSTERMS {tag} E32 {e32:.3e} kernel {err:.3e}")
    assert e32 < 1e-4, (tag, e32)
    assert err <= max(8.0 * e32, 1e-5), (tag, err, e32)


def _losses(tag, got, want):
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (tag, list(got), want)


def _compare(cad, dev, tag, inp, w, mask=None):
    """GPU against the float64 restatement at the module's bound; returns the GPU's (loss5, dpred)."""
    l64, d64 = _restate(*inp, w, mask)
    _, d32 = _restate(*inp, w, mask, dtype=torch.float32)
    l5, d = _gpu(cad, dev, w, *inp, mask=mask)
    assert torch.isfinite(d).all()
    _bound(tag, d, d64, d32)
    _losses(tag, l5, l64)
    return l5, d


@pytest.mark.parametrize("term", list(WEIGHTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_term_vs_fp64(cad, dev, shape, term):
    _compare(cad, dev, f"{term} {shape}", _inputs(*shape), WEIGHTS[term])


def test_mixed_is_the_sum_of_the_one_hot_runs(cad, dev):
    """dpred is linear in the weights: the mixed run against the GPU's own one-hot runs (the w2 == 0 early
    return of reduction 2 against its coupling path)."""
    inp = _inputs(2, 17, 65)
    parts = [_gpu(cad, dev, e, *inp)[1].double() for e in E]
    want = sum(float(np.float32(wi)) * p for wi, p in zip(MIXED, parts))
    got = _gpu(cad, dev, MIXED, *inp)[1]
    err = max_rel_err(got, want)
    print(f"LOSSTERMS linearity {err:.3e}")
    assert err <= 1e-6


def _clamp_inputs():
    """2 x 17 x 65 with pred planted on and across both clamp bounds.  Returns the inputs, the pixels where
    clamp() passes no gradient to pred itself, and the pixels where no scale of the pyramid passes one."""
    B, H, W = 2, 17, 65
    pred, gt, rgb, K = (a.copy() for a in _inputs(B, H, W))
    gt[gt == 0] = np.float32(2.5)                       # every planted pixel counts in SI / reprojection
    gt[:, :, :, 7::9] = 0                               # (holes elsewhere stay)
    vals = [0.0, -1.0, 1e-7, np.float32(1e-6), 1000.0, 1000.5, 5000.0]
    spots = [(0, 3, 5), (0, 5, 50), (0, 16, 64), (0, 9, 63), (0, 2, 64), (0, 16, 0), (0, 12, 41),
             (1, 9, 1), (1, 10, 26), (1, 16, 33), (1, 0, 0), (1, 15, 63), (1, 8, 64), (1, 11, 57)]
    for k, (b, y, x) in enumerate(spots):
        pred[b, 0, y, x] = np.float32(vals[(k + k // 7) % 7])
        gt[b, 0, y, x] = np.float32(3.0)
    pred[0, 0, 8:16, 16:24] = np.float32(1e-8)          # 8 x 8 block, every average below eps
    pred[0, 0, 0:8, 32:40] = 0.0                        # 8 x 8 block whose average alone is below eps:
    pred[0, 0, 3, 37] = np.float32(3e-5)                # 7.5e-6 at k = 2, 1.9e-6 at k = 4, 4.7e-7 at k = 8
    pred[1, 0, 0:8, 40:48] = (np.float32(1000.5) + np.float32(62.5) * np.arange(64, dtype=np.float32)).reshape(8, 8)
    own = (pred < np.float32(1e-6)) | (pred > np.float32(1000.0))
    every = np.zeros_like(own)
    every[0, 0, 8:16, 16:24] = True
    every[1, 0, 0:8, 40:48] = True
    return (pred, gt, rgb, K), own, every


@pytest.mark.parametrize("term", ["si", "grad", "reproj"])
def test_clamp_edges(cad, dev, term):
    """clamp(x, 1e-6, 1000) passes gradient on both bounds (inclusive).  Compared with the float32
    restatement: in float64 1e-6 and float(1e-6f) differ, so a pred of exactly 1e-6f falls on the other
    side.  E32 here is float32 against the float64 restatement with eps = float(1e-6f), the same constants
    in higher precision.  The few planted pixels just above eps carry gradients ~1e6 times the bulk and
    set the normalisation, so the bound is applied a second time over the pixels with pred >= 0.01."""
    inp, own, every = _clamp_inputs()
    w = WEIGHTS[term]
    l32, d32 = _restate(*inp, w, dtype=torch.float32)
    l64, d64 = _restate(*inp, w, eps=EPS32)
    l5, d = _gpu(cad, dev, w, *inp)
    assert torch.isfinite(d).all()
    e32 = max_rel_err(d32, d64)
    err = max_rel_err(d, d32)
    bulk = torch.from_numpy(inp[0] >= np.float32(0.01))
    e32b = max_rel_err(d32[bulk], d64[bulk])
    errb = max_rel_err(d.double()[bulk], d32[bulk])
    print(f"LOSSTERMS clamp {term} E32 {e32:.3e} kernel {err:.3e} bulk E32 {e32b:.3e} kernel {errb:.3e}")
    assert e32 < 1e-4 and e32b < 1e-4
    assert err <= max(8.0 * e32, 1e-5)
    assert errb <= max(8.0 * e32b, 1e-5)
    _losses(term, l5, l32)
    if term == "si":
        zero = torch.from_numpy(own)
    elif term == "grad":
        zero = torch.from_numpy(every)
    else:
        return   # the reprojection term has no clamp
    assert zero.sum() > 0 and (d32[zero] == 0).all()
    assert (d[zero] == 0).all()
    # the inclusive ends pass gradient: pred == 1e-6f and pred == 1000 exactly
    ends = torch.from_numpy((inp[0] == np.float32(1e-6)) | (inp[0] == np.float32(1000.0)))
    assert ends.sum() >= 4 and (d32[ends] != 0).all() and (d[ends] != 0).all()


def _tie_inputs():
    """2 x 32 x 64, pred and gt constant on 8 x 8 tiles with values k / 4 (exact in fp32, and so are the
    k x k sums of avg_pool2d): every difference inside a tile is exactly 0 at all four scales in either
    precision.  Sample 0's tiles (0..2, 0..2) share one value, so tile (1, 1) has no non-zero difference
    at any scale.  rgb is constant on the left half (exp(0) = 1 edges)."""
    B, H, W = 2, 32, 64
    from oracle.cad_oracle import u01
    k = (u01(0x71E5, np.arange(2 * B * 4 * 8, dtype=np.uint64)) * np.float32(36)).astype(np.int64).reshape(2, B, 4, 8)
    pt = (np.float32(0.75) + np.float32(0.25) * k[0]).astype(np.float32)
    gtile = (np.float32(0.5) + np.float32(0.25) * k[1]).astype(np.float32)
    gtile[:, 3, ::3] = 0                                   # hole tiles
    pt[0, 0:3, 0:3] = np.float32(2.25)
    gtile[0, 0:3, 0:3] = np.float32(1.75)
    up = lambda a: np.repeat(np.repeat(a, 8, axis=1), 8, axis=2).reshape(B, 1, H, W)
    _, _, rgb, K = _inputs(B, H, W)
    rgb = rgb.copy()
    rgb[:, :, :, : W // 2] = np.float32(0.5)
    return up(pt), up(gtile), rgb, K


@pytest.mark.parametrize("term", list(WEIGHTS))
def test_exact_ties(cad, dev, term):
    """sgn(0) = 0: flat regions.  Against float64 at the module's bound, and bit-exact where the gradient
    is a sum of sgn(0) terms.  Gradient matching: the pooled scales 2 and 3 see the tile edges from every
    pixel of a tile, so dpred is exactly 0 only on tile (1, 1) of sample 0's plateau; elsewhere the pixels
    2..5 of a tile have no scale-0 or scale-1 term, and those under one scale-2 cell must be bit-equal.
    Smoothness: tile-interior pixels hold only the uniform per-sample coupling, bit-equal within a sample."""
    inp = _tie_inputs()
    _, d = _compare(cad, dev, f"ties {term}", inp, WEIGHTS[term])
    d = d[:, 0]
    if term == "grad":
        assert d.abs().max() > 0
        assert (d[0, 8:16, 8:16] == 0).all()
        q = d.reshape(2, 4, 8, 8, 8).permute(0, 1, 3, 2, 4)   # (b, tile row, tile col, y in tile, x in tile)
        for ys in (slice(2, 4), slice(4, 6)):
            for xs in (slice(2, 4), slice(4, 6)):
                cell = q[..., ys, xs].reshape(2, 4, 8, 4)
                assert (cell == cell[..., :1]).all()
    if term == "smooth":
        q = d.reshape(2, 4, 8, 8, 8).permute(0, 1, 3, 2, 4)[..., 1:7, 1:7].reshape(2, -1)
        assert (q == q[:, :1]).all()
        assert (q[:, 0] != 0).all() and d.unique().numel() > 4   # the coupling is there, and edges differ


_MASK_SHAPE = (2, 17, 65)


def _mask_case(name):
    pred, gt, rgb, K = _inputs(*_MASK_SHAPE)
    B, H, W = _MASK_SHAPE
    if name == "all_holes":        # n = 0
        return (pred, np.zeros_like(gt), rgb, K), None
    if name == "one_valid":        # n = 1, in the one-lane column group
        m = np.zeros(gt.shape, bool)
        m[1, 0, 11, 64] = True
        assert gt[1, 0, 11, 64] > 0
        return (pred, gt, rgb, K), m
    if name == "holes_valid":      # the mask marks gt == 0 valid: log(1e-6) enters SI
        assert (gt == 0).sum() > 100
        return (pred, gt, rgb, K), np.ones(gt.shape, bool)
    if name == "mask_offcentre_K":  # cx, cy far outside the map, fx != fy, per sample
        from oracle.cad_oracle import u01
        m = u01(0x3A5C, np.arange(gt.size, dtype=np.uint64)).reshape(gt.shape) < np.float32(0.6)
        K = np.zeros((B, 3, 3), np.float32)
        K[0] = [[40.0, 0, -20.5], [0, 75.25, 3.0 * H], [0, 0, 1]]
        K[1] = [[91.5, 0, 2.0 * W], [0, 33.0, -7.75], [0, 0, 1]]
        return (pred, gt, rgb, K), m
    raise KeyError(name)


@pytest.mark.parametrize("term", ["si", "reproj", "mixed"])
@pytest.mark.parametrize("name", ["all_holes", "one_valid", "holes_valid", "mask_offcentre_K"])
def test_masks_and_counts(cad, dev, name, term):
    inp, mask = _mask_case(name)
    l5, d = _compare(cad, dev, f"{name} {term}", inp, WEIGHTS[term], mask)
    if name == "all_holes":
        assert l5[1] == 0 and l5[4] == 0
        if term != "mixed":
            assert l5[0] == 0 and (d == 0).all()
        else:   # gradient matching and smoothness are unaffected by n = 0
            assert l5[2] > 0 and l5[3] > 0 and (d != 0).any()


def test_forward_without_reprojection(cad, dev):
    """forward(): SI + gradient matching + smoothness through the lazily created second handle."""
    B, H, W = shape = (2, 24, 68)
    inp = _inputs(*shape)[:3] + (np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)),)   # forward() passes identity K
    w = MIXED[:3] + (0.0,)
    l64, d64 = _restate(*inp, w)
    _, d32 = _restate(*inp, w, dtype=torch.float32)
    loss = cad.CombinedDepthLoss(*MIXED, batch=B, height=H, width=W)
    assert loss.h_noreproj is None
    for _ in range(2):   # the call that creates the handle, and one that reuses it
        l5, d = loss.forward(_t(inp[0], dev), _t(inp[1], dev), _t(inp[2], dev))
        _bound("forward()", d.cpu(), d64, d32)
        _losses("forward()", l5.cpu().double().numpy(), l64)
    assert loss.h_noreproj is not None


def test_memory_discipline(cad, dev):
    """Inputs are the middle of larger allocations whose other rows are NaN, the handle is larger than the
    batch, dpred is twice the needed length: nothing outside the batch is read or written."""
    B, Bmax, H, W = 2, 4, 17, 65
    inp = _inputs(B, H, W)
    want5, wantd = _gpu(cad, dev, MIXED, *inp)

    def framed(a):   # [NaN sample | B samples | Bmax - B + 1 NaN samples], the batch as a view
        buf = torch.full((1 + Bmax + 1,) + a.shape[1:], float("nan"), device=dev)
        buf[1:1 + B] = _t(a, dev)
        return buf, buf[1:1 + B]
    bufs = [framed(a) for a in inp[:3]]
    n = B * H * W
    sentinel = -12345.5
    dbuf = torch.full((2 * n,), sentinel, device=dev)
    loss = cad.CombinedDepthLoss(*MIXED, batch=Bmax, height=H, width=W)
    l5, d = loss.forward_with_intrinsics(bufs[0][1], bufs[1][1], bufs[2][1], _t(inp[3], dev),
                                         dpred=dbuf[:n].view(B, 1, H, W))
    torch.cuda.synchronize()
    assert (dbuf[n:] == sentinel).all()
    assert torch.isfinite(dbuf[:n]).all() and (dbuf[:n] != sentinel).all()
    assert np.array_equal(l5.cpu().double().numpy(), want5) and torch.equal(d.cpu(), wantd)
    for (buf, _), a in zip(bufs, inp[:3]):   # the inputs are as they were
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[1 + B:]).all() and torch.equal(buf[1:1 + B].cpu(), torch.from_numpy(a))


def test_handle_reuse(cad, dev):
    """One handle through calls that leave different things in its workspace: each bit-equal to a fresh one."""
    B, H, W = 2, 33, 129
    pred, gt, rgb, K = _inputs(B, H, W)
    from oracle.cad_oracle import u01
    mask = u01(0x5EED, np.arange(gt.size, dtype=np.uint64)).reshape(gt.shape) < np.float32(0.5)
    calls = [((pred, gt, rgb, K), mask), ((pred, gt, rgb, K), None), ((pred, np.zeros_like(gt), rgb, K), None),
             ((pred[1:], gt[1:], rgb[1:], K[1:]), None)]
    loss = cad.CombinedDepthLoss(*MIXED, batch=B, height=H, width=W)
    for k, (inp, m) in enumerate(calls):
        a5, ad = _gpu(cad, dev, MIXED, *inp, mask=m, loss=loss)
        b5, bd = _gpu(cad, dev, MIXED, *inp, mask=m, max_batch=B)
        assert np.array_equal(a5, b5) and torch.equal(ad, bd), k


@pytest.mark.parametrize("max_batch,B,H,W", [(16, 15, 160, 224), (8, 7, 240, 320)])
def test_partial_batch_fits_the_workspace(cad, dev, max_batch, B, H, W):
    """B * ceil(2048 / B) blocks of partial sums can exceed max_batch * ceil(2048 / max_batch): the
    workspace is sized for every B <= max_batch, and the result is that of a handle made for B."""
    inp = _inputs(B, H, W)
    a5, ad = _gpu(cad, dev, MIXED, *inp, max_batch=max_batch)
    b5, bd = _gpu(cad, dev, MIXED, *inp, max_batch=B)
    assert np.isfinite(a5).all() and torch.isfinite(ad).all()
    assert np.array_equal(a5, b5) and torch.equal(ad, bd)


def test_sizes_below_16_are_refused(cad, dev):
    """Below 16 the k = 8 scale has no x or y difference (0/0): refused at creation, by value."""
    with pytest.raises(cad.CadError, match="height 15"):
        cad.CombinedDepthLoss(batch=1, height=15, width=64)
    with pytest.raises(cad.CadError, match="width 15"):
        cad.CombinedDepthLoss(batch=1, height=64, width=15)
    cad.CombinedDepthLoss(batch=1, height=16, width=16)
