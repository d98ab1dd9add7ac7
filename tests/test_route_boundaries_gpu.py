"""Kernel routes at their dispatch boundaries against float64.  The C-side pickers switch kernels at size limits (32-bit buffer
offsets of the 3x3 square-tile kernels at 2^31 bytes, 32-bit dropout indices of the split-bf16 attention at 4e9 scores, the tile counts
the feed-forward epilogues are instantiated for); every case asserts the route it lands on, so that it keeps covering that route if a
limit moves, and checks the result against float64 with the bounds of the per-kernel tests of the same kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import check_close

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _randn(shape, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(*shape, device=dev, generator=g)


def _picks(B):
    """the sampled images: the first, one in the middle, the last (whose offsets are the top of the range)"""
    return [0, B // 2, B - 1]


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _rel(got, want, norm=None):
    got, want = got.detach().double(), want.detach().double().to(got.device)
    return float((got - want).abs().max() / (want.abs().max() if norm is None else norm))


def _colsum64(t, step=256, square=False):
    """float64 per-channel sums (of squares) of an NHWC map, on the device, a slice of the batch at a time"""
    return sum((t[i:i + step].double() ** (2 if square else 1)).sum((0, 1, 2)) for i in range(0, t.shape[0], step))


def _report(case, **kw):
    print("\n[route-boundary] %s %s" % (case, " ".join("%s=%s" % (k, ("%.3e" % v) if isinstance(v, float) else v) for k, v in kw.items())))


def _zero_except(x, picks):
    """x = 0 except on the sampled images (a weight-gradient reference over those images alone; the kernel still walks the whole map)"""
    lo = 0
    for i in picks:
        x[lo:i].zero_()
        lo = i + 1
    x[lo:].zero_()


# ------------------------------------------------------------------------------------------- 3x3 convolutions at 2^31 bytes
@pytest.mark.parametrize("B,packing,wroute", [(4095, 14, 2), (4096, 10, 1)])
def test_conv3_chunked_relu_and_wgrad_either_side_of_2g(dev, B, packing, wroute):
    """Cin = Cout = 128 on 16 x 64 maps: B*H*W*128*4 = 2^31 - 2^19 bytes (square tiles, 32-bit offsets) / 2^31 (row tiles).  The
    contraction runs as two 64-channel chunks (beta = 1) and the ReLU acts on the whole sum on both routes.  The weight gradient and
    its bias gradient on the square-tile / row-segment kernels (x zero except on the sampled images)."""
    from tatt_amd import ops
    H, W, C = 16, 64, 128
    picks = _picks(B)
    g = torch.Generator().manual_seed(31)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g)
    wd, bd = w.to(dev), b.to(dev)
    x = _randn((B, H, W, C), dev, 1)
    xs = x[picks].cpu()
    ref = _nhwc(F.conv2d(_nchw(xs), w.double(), b.double(), padding=1))
    for act, want in ((ops.ACT_NONE, ref), (ops.ACT_RELU, torch.relu(ref))):
        assert ops.LIB.tatt_conv3_sb_packing(B, H, W, C, C, int(act), ops.ACT_NONE) == packing
        y = ops.conv2d_forward(x, wd, bd, act)
        err = _rel(y[picks].cpu(), want, ref.abs().max())
        del y
        _report("conv3 fwd C=128 B=%d" % B, act=act, packing=packing, err=err)
        assert err < 2e-5, (B, act, err)
    for act in (ops.ACT_NONE, ops.ACT_RELU):
        assert ops._conv3_sb_slices(x, C, C, act) == [(0, B)]            # one launch per chunk over the whole batch
    _zero_except(x, picks)
    dy = _randn((B, H, W, C), dev, 2)
    dw, db = ops.conv_wgrad(x, dy, C, 3, 3, want_db=True)
    ref_w = torch.nn.grad.conv2d_weight(_nchw(xs), (C, C, 3, 3), _nchw(dy[picks].cpu()), padding=1)
    err, errb = _rel(dw.cpu(), ref_w), _rel(db, _colsum64(dy))
    _report("conv3 wgrad C=128 B=%d" % B, route=wroute, err=err, errb=errb)
    del x, dy, dw, db
    _free()
    assert err < 2e-5, (B, "wgrad", err)
    assert errb < 2e-5, (B, "bias gradient", errb)
    assert ops.LIB.tatt_conv3_wgrad_sb_route(B, H, W, C, C) == wroute


@pytest.mark.parametrize("B,whole", [(10082, True), (10083, False)])
def test_conv3_ragged_width_either_side_of_2g(dev, B, whole):
    """The CRNN's ragged maps (any_width: 26-pixel rows, the last 16-pixel tile column cut by the map), 256 -> 256 channels on 8 rows:
    2,147,385,344 bytes (one launch on the square tiles) / 2,147,598,336 (beyond the limit only the row-tile kernels run, and they take
    W % 64 == 0: the batch runs as slices below the limit, each on the square tiles).  Forward with ReLU, data gradient, weight and bias
    gradient."""
    from tatt_amd import ops
    H, W, C = 8, 26, 256
    picks = _picks(B)
    g = torch.Generator().manual_seed(32)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g)
    wd, bd = w.to(dev), b.to(dev)
    x = _randn((B, H, W, C), dev, 3)
    xs = x[picks].cpu()
    ref = _nhwc(F.conv2d(_nchw(xs), w.double(), b.double(), padding=1))
    y = ops.conv2d_forward(x, wd, bd, ops.ACT_RELU, any_width=True)
    err = _rel(y[picks].cpu(), torch.relu(ref), ref.abs().max())
    del y
    _report("conv3 ragged fwd relu B=%d" % B, whole=whole, err=err)
    assert err < 2e-5, (B, "forward", err)
    dy = _randn((B, H, W, C), dev, 4)
    dys = dy[picks].cpu()
    dx = ops.conv2d_dgrad(dy, wd, any_width=True)
    ref_dx = _nhwc(torch.nn.grad.conv2d_input((3, C, H, W), w.double(), _nchw(dys), padding=1))
    err = _rel(dx[picks].cpu(), ref_dx)
    _report("conv3 ragged dgrad B=%d" % B, whole=whole, err=err)
    del dx
    assert err < 2e-5, (B, "dgrad", err)
    _zero_except(x, picks)
    dw, db = ops.conv_wgrad(x, dy, C, 3, 3, want_db=True, any_width=True)
    ref_w = torch.nn.grad.conv2d_weight(_nchw(xs), (C, C, 3, 3), _nchw(dys), padding=1)
    err, errb = _rel(dw.cpu(), ref_w), _rel(db, _colsum64(dy))
    _report("conv3 ragged wgrad B=%d" % B, whole=whole, err=err, errb=errb)
    assert err < 2e-5, (B, "wgrad", err)
    assert errb < 2e-5, (B, "bias gradient", errb)
    # the routes: the whole batch on the square tiles, or slices that each run there
    assert ops.LIB.tatt_conv3_sb_packing(B, H, W, C, C, ops.ACT_RELU, ops.ACT_NONE) == (14 if whole else 10)
    assert ops.LIB.tatt_conv3_sb_route(B, H, W, C, C, ops.ACT_RELU, ops.ACT_NONE) == (4 if whole else 0)
    assert ops.LIB.tatt_conv3_wgrad_sb_route(B, H, W, C, C) == (2 if whole else 0)
    for act in (ops.ACT_RELU, ops.ACT_NONE):
        sl = ops._conv3_sb_slices(x, C, C, act)
        assert (sl == [(0, B)]) == whole and sl[0][0] == 0 and sl[-1][1] == B
        assert all(ops.LIB.tatt_conv3_sb_route(b1 - b0, H, W, C, C, act, ops.ACT_NONE) == 4 for b0, b1 in sl)
    del x, dy, dw, db
    _free()


@pytest.mark.parametrize("B,packing", [(8191, 14), (8192, 10)])
def test_conv3_bn_forward_statistics_either_side_of_2g(dev, B, packing):
    """conv3_bn_forward, 64 -> 64 on 16 x 64 maps with the producer's BatchNorm + mish folded into the input and the output's batch
    statistics: 2^31 - 2^18 bytes (square tiles) / 2^31 (row tiles).  Values on the sampled images against float64; the statistics
    partials against float64 sums of the returned map."""
    from tatt_amd import ops
    H, W, C = 16, 64, 64
    picks = _picks(B)
    assert ops.LIB.tatt_conv3_sb_packing(B, H, W, C, C, ops.ACT_NONE, ops.ACT_NONE) == packing
    g = torch.Generator().manual_seed(33)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g)
    sc, sh = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    x = _randn((B, H, W, C), dev, 5)
    xs = x[picks].cpu()
    y, part, G = ops.conv3_bn_forward(x, w.to(dev), b.to(dev), sc.to(dev), sh.to(dev), ops.ACT_MISH, True)
    ref = _nhwc(F.conv2d(F.mish(_nchw(xs) * sc.double().view(1, C, 1, 1) + sh.double().view(1, C, 1, 1)), w.double(), b.double(),
                         padding=1))
    err = _rel(y[picks].cpu(), ref)
    st = part.view(G, 2, C).sum(0).cpu()
    s1, s2 = _colsum64(y).cpu(), _colsum64(y, square=True).cpu()
    del x, y, part
    _free()
    _report("conv3_bn_forward B=%d" % B, packing=packing, err=err, err_sum=float((st[0] - s1).abs().max() / s1.abs().max()),
            err_sq=float((st[1] - s2).abs().max() / s2.abs().max()))
    assert err < 2e-5, (B, err)
    check_close("stats.sum", st[0].float(), s1.float(), rtol=1e-5, atol=1e-3)
    check_close("stats.sq", st[1].float(), s2.float(), rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------------------- feed-forward on every prepacked width
def _ln1_64(t, gamma, beta, eps):
    """the TBSRN LayerNorm (layer-norm mode 1: unbiased std, eps added to the std)"""
    mu = t.mean(-1, keepdim=True)
    return gamma * (t - mu) / (t.std(-1, keepdim=True) + eps) + beta


@pytest.mark.parametrize("E,Nf", [(64, 64), (64, 128), (64, 192), (128, 64), (128, 128), (128, 192)])
@pytest.mark.parametrize("Pn", [320, 100])
@pytest.mark.parametrize("with_ln", [False, True])
def test_feed_forward_every_prepacked_width(dev, E, Nf, Pn, with_ln):
    """feed_forward / feed_forward_ln in training on every (d_model, d_ff) linear_prepack accepts, on a token count that is a multiple
    of 64 (B*P = 640) and one that is not (200).  The fused operators take the widths whose dropout / gate epilogues exist (d_ff <= 128);
    the rest runs the operator chain.  Dropout 0.1: fused == operator chain under the same seed; dropout 0: values and all gradients
    against float64 (pre-activations kept clear of zero, so that no relu decision is within rounding of flipping)."""
    from tatt_amd import functional as Fh
    B = 2
    fused_route = (B * Pn) % 64 == 0 and Nf <= 128
    g = torch.Generator().manual_seed(7 + E + Nf + Pn)
    x = torch.randn(B, Pn, E, generator=g)
    wo = torch.randn(B, Pn, E, generator=g)
    l1, l2 = torch.nn.Linear(E, Nf).to(dev), torch.nn.Linear(Nf, E).to(dev)
    with torch.no_grad():
        l1.weight.copy_(torch.randn(Nf, E, generator=g) * (0.05 / math.sqrt(E)))
        l1.bias.copy_(torch.sign(torch.randn(Nf, generator=g)) * (0.5 + torch.rand(Nf, generator=g)))
        l2.weight.copy_(torch.randn(E, Nf, generator=g) / math.sqrt(Nf))
        l2.bias.copy_(torch.randn(E, generator=g))
    ga, be = (torch.randn(E, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    fused_cls = Fh.FeedForwardLnFn if with_ln else Fh.FeedForwardFn

    def run(pdrop, fused):
        Fh.set_seed(dev, 9)
        Fh.begin_training_forward(dev)
        Fh.linear_prepack([l1, l2])
        Fh.FFN_FUSED = Fh.FFN_LN_FUSED = fused
        try:
            for t in (l1.weight, l1.bias, l2.weight, l2.bias, ga, be):
                t.grad = None
            xg = x.to(dev).requires_grad_(True)
            if with_ln:
                y = Fh.feed_forward_ln(xg, l1, l2, ga, be, 1e-6, 1, pdrop, True, 43)
            else:
                y = Fh.feed_forward(xg, l1, l2, pdrop, True, 41)
            assert isinstance(y.grad_fn, fused_cls._backward_cls) == (fused and fused_route), (fused, fused_route)
            (y * wo.to(dev)).sum().backward()
            out = [y, xg.grad, l1.weight.grad, l1.bias.grad, l2.weight.grad, l2.bias.grad] + ([ga.grad, be.grad] if with_ln else [])
            return [t.detach().cpu().clone() for t in out]
        finally:
            Fh.FFN_FUSED = Fh.FFN_LN_FUSED = True
            Fh.linear_prepack_done()

    names = ("y", "dx", "dw1", "db1", "dw2", "db2", "dgamma", "dbeta")
    a, c = run(0.1, True), run(0.1, False)
    for name, u, v in zip(names, a, c):
        assert float((u - v).abs().max()) <= 2e-6 * float(v.abs().max()), (name, float((u - v).abs().max()), float(v.abs().max()))
    assert float((a[0] - run(0.0, False)[0]).abs().max()) > 1e-3                # masks were applied
    got = run(0.0, True)
    xd = x.double().requires_grad_(True)
    W1, b1, W2, b2 = (t.detach().cpu().double().requires_grad_(True) for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    gd, bd = (t.detach().cpu().double().requires_grad_(True) for t in (ga, be))
    pre = F.linear(xd, W1, b1)
    assert float(pre.abs().min()) > 1e-3
    yr = F.linear(pre.clamp_min(0), W2, b2)
    if with_ln:
        yr = _ln1_64(xd + yr, gd, bd, 1e-6)
    (yr * wo.double()).sum().backward()
    want = [yr, xd.grad, W1.grad, b1.grad, W2.grad, b2.grad] + ([gd.grad, bd.grad] if with_ln else [])
    errs = {name: _rel(u, v) for name, u, v in zip(names, got, want)}
    _report("ffn E=%d Nf=%d M=%d ln=%d" % (E, Nf, B * Pn, with_ln), fused=fused_route, worst=max(errs.values()))
    for name, err in errs.items():
        assert err < 2e-5, (name, err)


# ------------------------------------------------------------------------------------------- self-attention routes
def _ref_attn64(q, k, v, h, keep=None, pdrop=0.0):
    """float64 attention of (n, P, E) tensors; keep (n, h, P, P) bool: the dropout mask (kept / (1 - p))"""
    n, Pn, E = q.shape
    d = E // h
    sp = lambda t: t.reshape(n, Pn, h, d).transpose(1, 2)
    p = torch.softmax(sp(q) @ sp(k).transpose(-2, -1) / d ** 0.5, -1)
    if keep is not None:
        p = p * keep / (1.0 - pdrop)
    return (p @ sp(v)).transpose(1, 2).reshape(n, Pn, E)


def _keep_mask(seed, site, pdrop, plane0, nplanes, Pn, dev):
    """dropout_keep (csrc/common.h) for the flat indices ((b h + head) P + q) P + key of planes [plane0, plane0 + nplanes), from the
    full 64-bit index: the high word enters as (idx >> 32) * 0x27D4EB2F"""
    k0 = (seed & M32) ^ ((site * 0x9E3779B9) & M32)
    k1 = ((seed >> 32) + site * 0x85EBCA77) & M32
    idx = torch.arange(nplanes * Pn * Pn, device=dev, dtype=torch.int64) + plane0 * Pn * Pn
    x = (((idx & M32) ^ k0) + (idx >> 32) * 0x27D4EB2F) & M32
    del idx
    x = ((x ^ (x >> 16)) * 0x85EBCA6B) & M32
    x = (x + k1) & M32
    x = ((x ^ (x >> 13)) * 0xC2B2AE35) & M32
    x = x ^ (x >> 16)
    return (x >= int(pdrop * 4294967296.0)).view(nplanes, Pn, Pn)


@pytest.fixture
def sattn_restore():
    from tatt_amd import functional as Fh
    old = (Fh.SATTN_SB, Fh.SATTN_KEEP_BITS, Fh.SATTN_FLASH, Fh.ATTN_LN_FUSED)
    yield
    Fh.SATTN_SB, Fh.SATTN_KEEP_BITS, Fh.SATTN_FLASH, Fh.ATTN_LN_FUSED = old
    Fh.ops.LIB.tatt_sattn_generation(2 if Fh.SATTN_SB else 1)


def _attn_run(dev, fn, base, w, pdrop, site, sb_fwd=True, sb_bwd=None):
    """fn(q, k, v, h = 4) under a fixed seed, SATTN_SB = sb_fwd in the forward and sb_bwd (default: unchanged) in the backward ->
    ([out, dq, dk, dv] on the host, the forward's ctx.cfg)"""
    from tatt_amd import functional as Fh
    Fh.set_seed(dev, 5)
    Fh.begin_training_forward(dev)
    Fh.SATTN_SB = sb_fwd
    try:
        q, k, v = (t.clone().to(dev).requires_grad_(True) for t in base)
        out = fn.apply(q, k, v, 4, pdrop, site)
        cfg = getattr(out.grad_fn, "cfg", None)
        if sb_bwd is not None:
            Fh.SATTN_SB = sb_bwd
        (out * w).sum().backward()
    finally:
        Fh.SATTN_SB = True
    return [t.detach().cpu() for t in (out, q.grad, k.grad, v.grad)], cfg


def _attn_holder(dev, E, h, seed):
    torch.manual_seed(seed)
    mh = torch.nn.Module()
    mh.h = h
    mh.linears = torch.nn.ModuleList([torch.nn.Linear(E, E) for _ in range(4)]).to(dev)
    return mh


def _attn_ln_run(dev, mh, ga, be, x, w, site, fused=True, sb_fwd=True, sb_bwd=None):
    """attention_ln in training (dropout 0.1) -> ([y, dx, dgamma, dbeta, the eight projection gradients] on the host, grad_fn)"""
    from tatt_amd import functional as Fh
    Fh.set_seed(dev, 6)
    Fh.begin_training_forward(dev)
    Fh.linear_prepack(list(mh.linears))
    Fh.ATTN_LN_FUSED = Fh.SATTN_FLASH = fused
    Fh.SATTN_SB = sb_fwd
    try:
        params = [ga, be] + [p for l in mh.linears for p in (l.weight, l.bias)]
        for t in params:
            t.grad = None
        xg = x.to(dev).requires_grad_(True)
        y = Fh.attention_ln(xg, mh, ga, be, 1e-6, 1, 0.1, site)
        if sb_bwd is not None:
            Fh.SATTN_SB = sb_bwd
        (y * w).sum().backward()
        return [t.detach().cpu().clone() for t in [y, xg.grad] + [p.grad for p in params]], y.grad_fn
    finally:
        Fh.ATTN_LN_FUSED = Fh.SATTN_FLASH = Fh.SATTN_SB = True
        Fh.linear_prepack_done()


@pytest.mark.parametrize("Pn", [64, 192, 320])
def test_flash_attention_dropout_beside_the_split_route(dev, Pn, sattn_restore):
    """Dropout on, P % 32 == 0 but P % 128 != 0: the split-bf16 kernels do not take the geometry, the exact-fp32 kernels run forward
    and backward and the forward allocates no keep bits.  SelfAttnFlashFn and attention_ln (AttnLnFn) against the materialised path
    under the same seed (bound 2e-5, as the fp32 route of the materialised-path test)."""
    from tatt_amd import functional as Fh
    B, E, h = 2, 128, 4
    g = torch.Generator().manual_seed(40 + Pn)
    base = [torch.randn(B, Pn, E, generator=g) for _ in range(3)]
    w = torch.randn(B, Pn, E, generator=g).to(dev)
    got, cfg = _attn_run(dev, Fh.SelfAttnFlashFn, base, w, 0.1, 77)
    want, _ = _attn_run(dev, Fh.SelfAttnCoreFn, base, w, 0.1, 77)
    errs = [float((a - c).abs().max()) / (float(c.abs().max()) + 1e-12) for a, c in zip(got, want)]
    _report("sattn P=%d flash vs materialised" % Pn, worst=max(errs))
    for name, err in zip(("out", "dq", "dk", "dv"), errs):
        assert err < 2e-5, (name, err)
    assert float((got[0] - _attn_run(dev, Fh.SelfAttnFlashFn, base, w, 0.0, 77)[0][0]).abs().max()) > 1e-3     # masks were applied
    mh = _attn_holder(dev, E, h, 43)
    ga, be = (torch.randn(E, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    res, fn = _attn_ln_run(dev, mh, ga, be, base[0], w, 50, fused=True)
    assert isinstance(fn, Fh.AttnLnFn._backward_cls)
    res_cfg = fn.cfg
    chain, fn = _attn_ln_run(dev, mh, ga, be, base[0], w, 50, fused=False)
    assert not isinstance(fn, Fh.AttnLnFn._backward_cls)
    # (index 7, W_k's bias gradient, is zero in exact arithmetic -- a shift of every score of a query by q.b_k leaves its softmax
    # unchanged -- so both paths leave round-off there: measured against the scale of W_k's weight gradient)
    errs = [float((a - c).abs().max()) / (float((chain[6] if k == 7 else c).abs().max()) + 1e-12) for k, (a, c) in enumerate(zip(res, chain))]
    _report("attention_ln P=%d fused vs chain" % Pn, worst=max(errs))
    for k, err in enumerate(errs):
        assert err < 2e-5, (k, err)
    assert not Fh.ops.LIB.tatt_sattn2_takes(B, Pn, h)
    assert cfg[5] is None and cfg[6] == 2 and res_cfg[5] is None and res_cfg[8] == 2    # no keep bits; the generation recorded


@pytest.mark.parametrize("sb_fwd,sb_bwd", [(True, False), (False, True)])
def test_flash_attention_backward_runs_the_forwards_route(dev, sb_fwd, sb_bwd, sattn_restore):
    """SATTN_SB flipped between forward and backward (P = 256, dropout on): the backward runs what its forward ran -- with the keep bits
    the split-bf16 forward filled, or recomputing the masks after an exact-fp32 forward that filled none -- so outputs and gradients
    equal the unflipped run's bit for bit; SelfAttnFlashFn and AttnLnFn."""
    from tatt_amd import functional as Fh
    B, Pn, E, h = 2, 256, 128, 4
    g = torch.Generator().manual_seed(41)
    base = [torch.randn(B, Pn, E, generator=g) for _ in range(3)]
    w = torch.randn(B, Pn, E, generator=g).to(dev)
    ref, cfg = _attn_run(dev, Fh.SelfAttnFlashFn, base, w, 0.1, 78, sb_fwd)
    got, _ = _attn_run(dev, Fh.SelfAttnFlashFn, base, w, 0.1, 78, sb_fwd, sb_bwd)
    for name, a, c in zip(("out", "dq", "dk", "dv"), got, ref):
        assert torch.equal(a, c), (name, float((a - c).abs().max()))
    mh = _attn_holder(dev, E, h, 44)
    ga, be = (torch.randn(E, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    ref_ln, fn = _attn_ln_run(dev, mh, ga, be, base[0], w, 51, True, sb_fwd)
    assert isinstance(fn, Fh.AttnLnFn._backward_cls)
    got_ln, _ = _attn_ln_run(dev, mh, ga, be, base[0], w, 51, True, sb_fwd, sb_bwd)
    for k, (a, c) in enumerate(zip(got_ln, ref_ln)):
        assert torch.equal(a, c), (k, float((a - c).abs().max()))
    assert (cfg[5] is not None) == sb_fwd and cfg[6] == (2 if sb_fwd else 1)


def test_flash_attention_keep_bits_with_indices_past_2_31(dev, sattn_restore):
    """h = 4, P = 4096 (TBSRN's reference geometry), B = 40: flat dropout indices up to 2.7e9, past 2^31, on the split-bf16 route.
    Every keep bit of the last (b, head) plane against the counter hash; gradients with the keep bits and with recomputed masks:
    values, dK and dV equal bit for bit, dQ to 2e-5."""
    from tatt_amd import ops
    from tatt_amd import functional as Fh
    B, Pn, E, h, site, pdrop = 40, 4096, 128, 4, 100, 0.1
    assert (B * h - 1) * Pn * Pn > 2 ** 31
    Q, K, V = (_randn((B, Pn, E), dev, 60 + i) for i in range(3))
    seed = 0x7FEDCBA987654321
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    ops.LIB.tatt_sattn_generation(2)
    O, lse = torch.empty_like(Q), torch.empty(B, h, Pn, device=dev)
    bits = torch.zeros(B * h * Pn * Pn // 32, device=dev, dtype=torch.int32)
    ops.call("tatt_sattn_fwd_bits", ops.P(Q), ops.P(K), ops.P(V), ops.P(O), ops.P(lse), ops.P(bits), B, Pn, h, 32 ** -0.5, pdrop, ops.P(sd),
             site, ops.stream())
    keep = _keep_mask(seed, site, pdrop, B * h - 1, 1, Pn, dev)[0]
    nb = Pn // 32
    words = bits.view(B * h, nb, nb, 32)[-1].to(torch.int64) & M32       # [query block][key block][word]
    got = torch.zeros_like(keep)
    for d in range(32):
        vv, half = d >> 1, d & 1
        key = (vv & 3) + 8 * (vv >> 2) + 4 * half
        for qq in range(32):
            got[qq::32, key::32] = ((words[:, :, d] >> qq) & 1).bool()
    assert torch.equal(got, keep), int((got != keep).sum())
    assert 0.88 < float(got.float().mean()) < 0.92
    del bits, words, got, keep, O, lse
    w = _randn((B, Pn, E), dev, 63)
    res, cfgs = [], []
    for keep_bits in (True, False):
        Fh.SATTN_KEEP_BITS = keep_bits
        r, cfg = _attn_run(dev, Fh.SelfAttnFlashFn, (Q, K, V), w, pdrop, 79)
        res.append(r)
        cfgs.append((cfg[5] is not None, cfg[6] if len(cfg) > 6 else None))
    a, b = res
    _report("sattn B=40 P=4096 keep bits on/off", dq=float((a[1] - b[1]).abs().max()) / float(b[1].abs().max()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert float((a[1] - b[1]).abs().max()) / float(b[1].abs().max()) < 2e-5
    _free()
    assert ops.LIB.tatt_sattn2_takes(B, Pn, h) and cfgs == [(True, 2), (False, 2)]


@pytest.mark.parametrize("B,split", [(59, True), (60, False)])
def test_flash_attention_either_side_of_4e9_scores(dev, B, split, sattn_restore):
    """h = 4, P = 4096: B h P^2 = 3.96e9 (split bf16) / 4.03e9 (the exact-fp32 kernels), dropout off: values and the Q / K / V gradients
    of the first and the last batch item against float64 attention (bounds 1e-4 split, 2e-5 fp32)."""
    from tatt_amd import functional as Fh
    Pn, E, h = 4096, 128, 4
    Q, K, V, w = (_randn((B, Pn, E), dev, 70 + i) for i in range(4))
    got, cfg = _attn_run(dev, Fh.SelfAttnFlashFn, (Q, K, V), w, 0.0, 0)
    bound = 1e-4 if split else 2e-5
    errs = {}
    for i in (0, B - 1):
        qd, kd, vd = (t[i:i + 1].double().requires_grad_(True) for t in (Q, K, V))
        ref = _ref_attn64(qd, kd, vd, h)
        (ref * w[i:i + 1].double()).sum().backward()
        for name, a, c in zip(("out", "dq", "dk", "dv"), got, (ref, qd.grad, kd.grad, vd.grad)):
            errs[(i, name)] = _rel(a[i:i + 1], c.cpu())
        del qd, kd, vd, ref
    _free()
    _report("sattn B=%d P=4096 vs fp64" % B, split=split, worst=max(errs.values()))
    assert max(errs.values()) < bound, errs
    assert bool(Fh.ops.LIB.tatt_sattn2_takes(B, Pn, h)) == split and cfg[5] is None and cfg[6] == 2


def test_flash_attention_dropout_indices_past_2_32(dev, sattn_restore):
    """h = 4, P = 4096, B = 65 (the exact-fp32 kernels): the last batch item's flat dropout indices pass 2^32, where dropout_keep mixes
    in the high word.  Its values and gradients against float64 attention under the mask built from the full 64-bit index."""
    from tatt_amd import functional as Fh
    B, Pn, E, h, pdrop, site = 65, 4096, 128, 4, 0.1, 80
    assert (B - 1) * h * Pn * Pn >= 2 ** 32
    Q, K, V, w = (_randn((B, Pn, E), dev, 80 + i) for i in range(4))
    Fh.set_seed(dev, 5)
    Fh.begin_training_forward(dev)
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = Fh.SelfAttnFlashFn.apply(q, k, v, h, pdrop, site)
    cfg = out.grad_fn.cfg
    seed = int(cfg[3].item()) & 0xFFFFFFFFFFFFFFFF
    (out * w).sum().backward()
    i = B - 1
    keep = _keep_mask(seed, site, pdrop, i * h, h, Pn, dev).view(1, h, Pn, Pn)
    assert 0.88 < float(keep.float().mean()) < 0.92
    qd, kd, vd = (t[i:i + 1].double().requires_grad_(True) for t in (Q, K, V))
    ref = _ref_attn64(qd, kd, vd, h, keep, pdrop)
    (ref * w[i:i + 1].double()).sum().backward()
    errs = {name: _rel(a[i:i + 1], c) for name, a, c in zip(("out", "dq", "dk", "dv"), (out, q.grad, k.grad, v.grad),
                                                             (ref, qd.grad, kd.grad, vd.grad))}
    del keep, ref, qd, kd, vd
    _free()
    _report("sattn B=65 P=4096 dropout vs fp64", worst=max(errs.values()))
    assert max(errs.values()) < 2e-5, errs
    assert not Fh.ops.LIB.tatt_sattn2_takes(B, Pn, h) and cfg[5] is None and cfg[6] == 2
