"""The kernels of the step's single-lane stretches, each through its C entry point at the smallest shapes that reach every route:
PixelShuffle(2) + activation (quad route and the per-element route behind it), ImageLoss (sr quads over NHWC memory and the strided
route; the forward's wave sums finished by a second launch), the fully connected pair of the STN head at partial 16-row tiles and at
its bound, and the key / value projections of tatt_tplayer2_kvprep.  References: torch's own pixel_shuffle, the CPU oracle, float64."""
import pytest
import torch
import torch.nn.functional as F

from oracle import tatt_oracle as O
from tests.util import check_close, max_err

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_MISH = 0, 2


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------------------------ PixelShuffle
def _shifted(t):
    """the same values in memory that starts 4 bytes after an allocation: no longer 16-byte aligned"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _unshuffle(dout):
    """inverse permutation of PixelShuffle(2) on NHWC maps: (B, 2H, 2W, C) -> (B, H, W, 4C)"""
    return F.pixel_unshuffle(dout.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 3, 5, 64), (1, 2, 3, 6)])      # C = 6: the per-element route
def test_pixel_shuffle_routes(dev, B, H, W, C, shift):
    from tatt_amd import ops
    x = _rand(B, H, W, 4 * C, seed=1).to(dev)
    dout = _rand(B, 2 * H, 2 * W, C, seed=2).to(dev)
    if shift:
        x, dout = _shifted(x), _shifted(dout)
    # no activation: the permutation alone, exact
    y = ops.pixel_shuffle_fwd(x, ACT_NONE)
    assert torch.equal(y, F.pixel_shuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    assert torch.equal(ops.pixel_shuffle_bwd(x, dout, ACT_NONE), _unshuffle(dout))
    # mish: the activation commutes with the permutation, value for value
    assert torch.equal(ops.pixel_shuffle_fwd(x, ACT_MISH), ops.pixel_shuffle_fwd(ops.act_fwd(x.contiguous(), ACT_MISH), ACT_NONE))
    # backward: dout (unshuffled) times act_bwd's factor.  Both kernels evaluate common.h's act_grad and take one fp32 product with it;
    # the bound leaves room for one rounding of difference (a multiply-add contracted in one kernel and not in the other): 2^-22 relative
    got = ops.pixel_shuffle_bwd(x, dout, ACT_MISH)
    ref = ops.act_bwd(x.contiguous(), _unshuffle(dout), ACT_MISH, False)
    err = (got - ref).abs()
    assert bool((err <= 2.0 ** -22 * ref.abs() + 1e-30).all()), float(err.max())


# --------------------------------------------------------------------------------------------------------------------- ImageLoss
@pytest.mark.parametrize("B,C,H,W,nhwc", [(1, 1, 3, 3, False), (2, 4, 1, 5, False), (2, 3, 8, 16, False), (3, 4, 32, 128, True),
                                          (2, 4, 3, 5, True)])
def test_image_loss_routes(dev, B, C, H, W, nhwc):
    """loss, scaled mean and both gradient forms against the oracle with the bounds of test_image_loss_fused; a second call returns
    the same bits (the wave sums are added in a fixed order)"""
    from tatt_amd.train import image_loss, image_loss_mean
    g = torch.Generator().manual_seed(41 + H)
    sr = (torch.rand(B, C, H, W, generator=g) * 2 - 1).requires_grad_(True)
    hr = torch.rand(B, C, H, W, generator=g)
    wts = torch.rand(B, generator=g)
    ref = O.image_loss(sr, hr)
    (ref * wts).sum().backward()
    srd = sr.detach().to(dev)
    if nhwc:
        srd = srd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    srd.requires_grad_(True)
    hrd = hr.to(dev)
    got = image_loss(srd, hrd)
    check_close("image_loss", got, ref, 1e-5, 1e-7)
    (got * wts.to(dev)).sum().backward()
    check_close("image_loss_grad", srd.grad, sr.grad, 2e-4, 1e-9)
    g_per = srd.grad.clone()
    srd.grad = None
    sr.grad = None
    (O.image_loss(sr, hr).mean() * 100).backward()
    m = image_loss_mean(srd, hrd, scale=100.0)
    assert abs(float(m) - float(ref.mean() * 100)) < 1e-5 * float(ref.mean() * 100)
    m.backward()
    check_close("image_loss_mean_grad", srd.grad, sr.grad, 2e-4, 1e-9)
    g_mean = srd.grad.clone()
    # again: the same bits
    srd.grad = None
    got2 = image_loss(srd, hrd)
    (got2 * wts.to(dev)).sum().backward()
    assert torch.equal(got2, got) and torch.equal(srd.grad, g_per)
    srd.grad = None
    m2 = image_loss_mean(srd, hrd, scale=100.0)
    m2.backward()
    assert torch.equal(m2, m) and torch.equal(srd.grad, g_mean)


# ------------------------------------------------------------------------------------------- fully connected pair of the STN head
def _fc_reference(t, B, dctrl, eps, momentum):
    """Linear(512, 512) on the flattened (B, 256, 1, 2) map -> BatchNorm1d (batch statistics) -> ReLU -> x 0.1 -> Linear(512, NO), forward
    and backward in the dtype of `t` (dict of leaf tensors).  The BatchNorm is written out, so that B = 1 has a defined result."""
    t = {k: v.detach().clone().requires_grad_(k not in ("rm", "rv")) for k, v in t.items()}
    Fm = t["A6"].permute(0, 2, 1).reshape(B, 512)                          # feature c * 2 + w of the NCHW flattening is A6[b][w][c]
    U = Fm @ t["W1"].t() + t["b1"]
    U.retain_grad()
    mu = U.mean(0)
    var = ((U - mu) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    S = 0.1 * torch.relu((U - mu) * rstd * t["g1"] + t["be1"])
    ctrl = S @ t["W2"].t() + t["b2"]
    ctrl.backward(dctrl.to(ctrl.dtype))
    unb = var * (B / (B - 1)) if B > 1 else var
    out = {"ctrl": ctrl, "U": U, "S": S, "mean1": mu, "rstd1": rstd, "rm": (1 - momentum) * t["rm"] + momentum * mu,
           "rv": (1 - momentum) * t["rv"] + momentum * unb, "dU": U.grad, "dA6": t["A6"].grad, "dW1": t["W1"].grad,
           "db1": t["b1"].grad, "dg1": t["g1"].grad, "dbe1": t["be1"].grad, "dW2": t["W2"].grad, "db2": t["b2"].grad}
    return {k: v.detach() for k, v in out.items()}


def _fc_hip(t, B, NO, dctrl, eps, momentum, dev):
    from tatt_amd import ops, functional as Fh
    Fh.sticky_word(dev)
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    new = lambda *s: torch.empty(*s, device=dev)
    U, S, mean1, rstd1, ctrl = new(B, 512), new(B, 512), new(512), new(512), new(B, NO)
    part = new(32 * B * NO)
    sync_f = torch.zeros(256, dtype=torch.int32, device=dev)
    sync_b = torch.zeros(256, dtype=torch.int32, device=dev)
    P = ops.P
    ops.call("tatt_stn_fc_fwd", P(d["A6"]), P(d["W1"]), P(d["b1"]), P(d["g1"]), P(d["be1"]), P(d["rm"]), P(d["rv"]), P(d["W2"]), P(d["b2"]),
             P(U), P(mean1), P(rstd1), P(S), P(ctrl), P(part), P(sync_f), B, NO, eps, momentum, ops.stream())
    dc = dctrl.to(dev).contiguous()
    dW2, db2, dg1, dbe1 = torch.empty_like(d["W2"]), torch.empty_like(d["b2"]), new(512), new(512)
    dW1, db1, dU, dA6 = torch.empty_like(d["W1"]), new(512), new(B, 512), torch.empty_like(d["A6"])
    ops.call("tatt_stn_fc_bwd", P(dc), P(d["W2"]), P(S), P(U), P(mean1), P(rstd1), P(d["g1"]), P(d["W1"]), P(d["A6"]), P(dW2), P(db2), P(dg1),
             P(dbe1), P(dW1), P(db1), P(dU), P(dA6), P(sync_b), B, NO, ops.stream())
    torch.cuda.synchronize()
    Fh.sync_check()
    assert int(sync_f[255].item()) == 0 and int(sync_b[255].item()) == 0          # no launch gave up waiting
    out = {"ctrl": ctrl, "U": U, "S": S, "mean1": mean1, "rstd1": rstd1, "rm": d["rm"], "rv": d["rv"], "dU": dU, "dA6": dA6, "dW1": dW1,
           "db1": db1, "dg1": dg1, "dbe1": dbe1, "dW2": dW2, "db2": db2}
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("B", [1, 5, 17, 48, 64])
def test_stn_fc_pair_against_float64(dev, B):
    """tatt_stn_fc_fwd / tatt_stn_fc_bwd alone: every output and parameter gradient against float64 with the bound test_stn_gpu.py holds
    the fused head to (4 x the distance of the same operators in plain fp32 + 2e-5, relative to the largest reference entry; the bias
    in front of the BatchNorm has a mathematically zero gradient and is bounded as there).  A second run returns the same bits."""
    NO, eps, momentum = 40, 1e-5, 0.1
    g = torch.Generator().manual_seed(100 + B)
    r = lambda *s: torch.randn(*s, generator=g)
    t = {"A6": torch.relu(r(B, 2, 256)), "W1": 0.03 * r(512, 512), "b1": 0.2 * r(512), "g1": 1.0 + 0.2 * r(512), "be1": 0.2 * r(512),
         "W2": 0.05 * r(NO, 512), "b2": r(NO), "rm": 0.1 * r(512), "rv": 1.0 + 0.1 * torch.rand(512, generator=g)}
    dctrl = r(B, NO)
    ref = _fc_reference({k: v.double() for k, v in t.items()}, B, dctrl, eps, momentum)
    f32 = _fc_reference(t, B, dctrl, eps, momentum)
    got = _fc_hip(t, B, NO, dctrl, eps, momentum, dev)
    again = _fc_hip(t, B, NO, dctrl, eps, momentum, dev)
    assert set(got) == set(ref)
    for k in sorted(ref):
        assert torch.equal(got[k], again[k]), k
        if k == "db1":
            lim = 1e-4 * float(ref["dW1"].abs().max()) * (B * 16 * 64) ** 0.5
            assert float(got[k].abs().max()) <= lim, (k, float(got[k].abs().max()), lim)
            continue
        scale = float(ref[k].abs().max()) + 1e-30
        e_f32 = float((f32[k].double() - ref[k]).abs().max()) / scale
        e_hip = float((got[k].double() - ref[k]).abs().max()) / scale
        assert e_hip <= 4.0 * e_f32 + 2e-5, (k, e_hip, e_f32)


# ------------------------------------------------------------------------------------------------------------------------ kvprep
@pytest.mark.parametrize("B,S,nl", [(1, 1, 1), (3, 26, 2), (2, 32, 2)])
def test_kvprep_projections_against_float64(dev, B, S, nl):
    """tatt_tplayer2_kvprep: kin = mem + pos exactly, and the fp32 key / value images unpacked ([form][h][i2][lane][u]: keys as
    K[16 i2 + am][16 h + 4 kq + u], values as V[16 i2 + 4 kq + u][16 h + am], rows >= S zero) against float64 projections with the
    bound test_tplayer_gpu.py holds them to (2e-6 of the largest entry); pos shared by the batch and per sample."""
    from tatt_amd import ops
    g = torch.Generator().manual_seed(11 + S)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.4)
    mem = r(B, S, 64)
    lps = [tuple(r(*s) for s in ((192, 64), (192,), (64, 64), (64,), (64, 64), (64,), (64, 64), (64,), (64,), (64,), (64,), (64,)))
           for _ in range(nl)]
    lane = torch.arange(64)
    am, kq = lane & 15, lane >> 4
    h, i2, u = torch.arange(4), torch.arange(2), torch.arange(4)
    # [h][i2][lane][u] index grids
    k_row = (16 * i2[None, :, None, None] + am[None, None, :, None]).expand(4, 2, 64, 4)
    k_col = (16 * h[:, None, None, None] + 4 * kq[None, None, :, None] + u[None, None, None, :]).expand(4, 2, 64, 4)
    v_row = (16 * i2[None, :, None, None] + 4 * kq[None, None, :, None] + u[None, None, None, :]).expand(4, 2, 64, 4)
    v_col = (16 * h[:, None, None, None] + am[None, None, :, None]).expand(4, 2, 64, 4)
    for pos in (r(S, 64), r(B, S, 64)):
        kin, packs = ops.tplayer2_kvprep(mem.to(dev), pos.to(dev), [tuple(x.to(dev) for x in lp) for lp in lps])
        kin64 = mem.double() + pos.double()
        assert torch.equal(kin.cpu(), kin64.float())
        for lp, pk in zip(lps, packs):
            w, bias = lp[0].double(), lp[1].double()
            K = torch.zeros(B, 32, 64, dtype=torch.float64)
            V = torch.zeros(B, 32, 64, dtype=torch.float64)
            K[:, :S] = kin64.float().double() @ w[64:128].t() + bias[64:128]
            V[:, :S] = mem.double() @ w[128:].t() + bias[128:]
            ref = torch.stack([K[:, k_row, k_col], V[:, v_row, v_col]], 1)                   # (B, 2, 4, 2, 64, 4)
            img = pk[3].cpu().reshape(B, 2, 4, 2, 64, 4)
            assert max_err(img, ref) <= 2e-6 * float(ref.abs().max())
