"""The float64 specifications of tests/norm_attn_ref.py against torch's own float64 operators and float64 autograd, on the CPU: a mistake
in a reference must not hide one in a kernel.  Limit: 1e-12 relative to the largest |value| of the compared tensor."""
import pytest
import torch
import torch.nn.functional as F

from oracle import tatt_oracle as O
from tests import norm_attn_ref as NR

LIMIT = 1e-12
D = torch.float64


def close(got, want, what=""):
    assert got.shape == want.shape and got.dtype == D and want.dtype == D, what
    top = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= LIMIT * top, (what, err, top)


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=D)


def mask_of(gen, shape, p=0.1):
    return (torch.rand(shape, generator=gen) >= p).to(D) / (1.0 - p)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_activations(act):
    u = torch.linspace(-30, 30, 2001, dtype=D).requires_grad_()
    want = [lambda t: t, torch.relu, F.mish][act](u)
    y = NR.act_fn(u, act)
    close(y.detach(), want.detach())
    (g,) = torch.autograd.grad(want.sum(), u)
    close(NR.act_grad(u.detach(), act), g)
    close(NR.act_fn(u.detach(), act), O.mish(u.detach()) if act == 2 else want.detach())


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,C", [(2, 3), (5, 1), (63, 37), (257, 16)])
def test_batchnorm(training, act, M, C):
    gen = torch.Generator().manual_seed(M * 100 + C)
    x = (1.5 * rnd(gen, M, C) + 0.3).requires_grad_()
    gamma, beta = (1 + 0.3 * rnd(gen, C)).requires_grad_(), (0.2 * rnd(gen, C)).requires_grad_()
    rm, rv = 0.4 * rnd(gen, C), 0.5 + torch.rand(C, generator=gen, dtype=D)
    dy = rnd(gen, M, C)
    actf = [lambda t: t, torch.relu, F.mish][act]
    trm, trv = rm.clone(), rv.clone()
    want = actf(F.batch_norm(x, trm, trv, gamma, beta, training, 0.1, 1e-5))
    y, mean, rstd, nrm, nrv = NR.bn_forward(x.detach(), gamma.detach(), beta.detach(), rm, rv, training, 0.1, 1e-5, act)
    close(y, want.detach(), "y")
    close(nrm, trm, "running_mean"), close(nrv, trv, "running_var")
    if training:
        close(mean, x.detach().mean(0)), close(rstd, 1.0 / torch.sqrt(x.detach().var(0, unbiased=False) + 1e-5))
    else:
        assert torch.equal(nrm, rm) and torch.equal(nrv, rv)
    wdx, wdg, wdb = torch.autograd.grad((want * dy).sum(), [x, gamma, beta])
    dx, dg, db = NR.bn_backward(x.detach(), dy, mean, rstd, gamma.detach(), beta.detach(), act, training)
    # (the backward formula cancels: its error is relative to the terms it subtracts, gamma rstd |du|)
    top = float((gamma.detach() * rstd).abs().max() * dy.abs().max())
    assert float((dx - wdx).abs().max()) <= LIMIT * max(top, float(wdx.abs().max()))
    close(dg, wdg, "dgamma"), close(db, wdb, "dbeta")
    # the three-piece form equals the one-piece form
    du, xh, s, q = NR.bn_partial_sums(x.detach(), dy, mean, rstd, gamma.detach(), beta.detach(), act)
    dg3, db3, coef = NR.bn_backward_finish(s, q, M, mean, rstd, gamma.detach())
    assert torch.equal(dg3, dg) and torch.equal(db3, db)
    if training:
        dx3 = NR.bn_backward_affine(x.detach(), du, coef)
        assert float((dx3 - wdx).abs().max()) <= LIMIT * max(top * float(1 + x.detach().abs().max() * rstd.max()), float(wdx.abs().max()))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("residual", ["none", "plain", "dropped"])
@pytest.mark.parametrize("M,C", [(1, 2), (5, 37), (4, 64), (3, 256)])
def test_layernorm(mode, residual, M, C):
    gen = torch.Generator().manual_seed(M * 1000 + C)
    a = rnd(gen, M, C).requires_grad_()
    b = rnd(gen, M, C).requires_grad_() if residual != "none" else None
    mask = mask_of(gen, (M, C)) if residual == "dropped" else None
    gamma, beta = (1 + 0.3 * rnd(gen, C)).requires_grad_(), (0.2 * rnd(gen, C)).requires_grad_()
    eps = 1e-5 if mode == 0 else 1e-6
    dy = rnd(gen, M, C)
    x = a if b is None else a + (b if mask is None else b * mask)
    want = F.layer_norm(x, (C,), gamma, beta, eps) if mode == 0 else O.tbsrn_layer_norm(x, gamma, beta, eps)
    det = lambda t: None if t is None else t.detach()
    close(NR.layer_norm(det(a), det(b), det(gamma), det(beta), eps, mode, mask), want.detach(), "y")
    leaves = [a, gamma, beta] + ([b] if b is not None else [])
    grads = torch.autograd.grad((want * dy).sum(), leaves)
    dx, db, dg, dbeta = NR.layer_norm_backward(det(a), det(b), dy, det(gamma), eps, mode, mask)
    # (cancelling formula: relative to rs |g|, the terms it subtracts)
    rs = NR._ln_parts(det(a), det(b), eps, mode, mask)[1]
    top = float(rs.max() * (dy * det(gamma)).abs().max())
    assert float((dx - grads[0]).abs().max()) <= LIMIT * top
    close(dg, grads[1], "dgamma"), close(dbeta, grads[2], "dbeta")
    if b is None:
        assert db is None
    else:
        assert float((db - grads[3]).abs().max()) <= LIMIT * top * (1.0 / 0.9)


@pytest.mark.parametrize("B,Lq,S", [(1, 1, 1), (2, 5, 32), (3, 65, 17)])
@pytest.mark.parametrize("dropped", [False, True])
def test_attention_core(B, Lq, S, dropped):
    gen = torch.Generator().manual_seed(B * 100 + Lq + S)
    Q, K, V = rnd(gen, B, Lq, 64), rnd(gen, B, S, 64), rnd(gen, B, S, 64)
    mask = mask_of(gen, (B, 4, Lq, S)) if dropped else None
    ctx, wavg = NR.attn_core(Q, K, V, mask)
    # an explicit loop over images and heads
    wc, ww = torch.zeros(B, Lq, 64, dtype=D), torch.zeros(B, Lq, S, dtype=D)
    for b in range(B):
        for h in range(4):
            cols = slice(16 * h, 16 * h + 16)
            p = torch.softmax(Q[b, :, cols] @ K[b, :, cols].t(), -1)
            if mask is not None:
                p = p * mask[b, h]
            wc[b, :, cols] = p @ V[b, :, cols]
            ww[b] += p / 4
    close(ctx, wc, "ctx"), close(wavg, ww, "wavg")
    if not dropped:
        # nn.MultiheadAttention with identity projections scales q by 1 / sqrt(16) itself: hand it 4 Q
        eye, zero = torch.eye(64, dtype=D).repeat(3, 1), torch.zeros(192, dtype=D)
        o, w = F.multi_head_attention_forward((4.0 * Q).transpose(0, 1), K.transpose(0, 1), V.transpose(0, 1), 64, 4, eye, zero, None, None,
                                              False, 0.0, torch.eye(64, dtype=D), torch.zeros(64, dtype=D), training=False,
                                              need_weights=True)
        close(ctx, o.transpose(0, 1).contiguous(), "ctx vs mha"), close(wavg, w, "wavg vs mha")
        assert float((wavg.sum(-1) - 1).abs().max()) < 1e-12
    # large scores: finite thanks to the max subtraction
    c2, w2 = NR.attn_core(200.0 * Q, K, V, mask)
    assert bool(torch.isfinite(c2).all()) and bool(torch.isfinite(w2).all())


@pytest.mark.parametrize("rows,L", [(1, 1), (3, 37), (2, 4096)])
def test_softmax_rows(rows, L):
    gen = torch.Generator().manual_seed(rows + L)
    S = 3.0 * rnd(gen, rows, L)
    S[0] += 80.0
    mask = mask_of(gen, (rows, L))
    p, pd = NR.softmax_rows(S, mask)
    close(p, torch.softmax(S, -1)), close(pd, torch.softmax(S, -1) * mask)
    p0, pd0 = NR.softmax_rows(S, None)
    assert pd0 is p0 and torch.equal(p0, p)
    # the backward the kernel implements, dS = P (g - sum P g) with g = mask dPd, equals float64 autograd of the specification
    Sg = S.clone().requires_grad_()
    dPd = rnd(gen, rows, L)
    (NR.softmax_rows(Sg, mask)[1] * dPd).sum().backward()
    g = dPd * mask
    want = p * (g - (p * g).sum(-1, keepdim=True))
    assert float((Sg.grad - want).abs().max()) <= 1e-12 * float(g.abs().max())


@pytest.mark.parametrize("B,N,P", [(1, 1, 1), (3, 20, 35), (2, 29, 257)])
def test_tps_grid(B, N, P):
    gen = torch.Generator().manual_seed(N + P)
    ctrl, inv, pad, rep = rnd(gen, B, N, 2), rnd(gen, N + 3, N + 3), rnd(gen, 3, 2), rnd(gen, P, N + 3)
    got = NR.tps_grid(ctrl, inv, pad, rep)
    for b in range(B):
        close(got[b], rep @ (inv @ torch.cat([ctrl[b], pad], 0)))
    # the expression of the oracle (tps_transform): mapping = inverse_kernel @ Y, source = repr @ mapping
    Y = torch.cat([ctrl, pad.expand(B, 3, 2)], 1)
    close(got, torch.matmul(rep, torch.matmul(inv, Y)))


@pytest.mark.parametrize("C,H,W,B", [(1, 1, 1, 1), (3, 5, 7, 3), (4, 16, 64, 1), (1, 16, 64, 3), (4, 1, 1, 3)])
def test_grid_sample(C, H, W, B):
    x, src, dout = NR.sample_inputs(B, C, H, W, seed=C * 1000 + H * W + B)
    x, dout = x.double(), dout.double()
    src = src.double().requires_grad_()
    assert bool((src.detach() == 0).any()) and (src.numel() == 2 or bool((src.detach() == 1).any()))
    assert float(src.detach().min()) < 0 or src.numel() < 8
    got = NR.grid_sample_nhwc(x, src)
    s2 = src.detach().clone().requires_grad_()
    want = F.grid_sample(x, (2.0 * torch.clamp(s2, 0.0, 1.0) - 1.0).view(B, H, W, 2), mode="bilinear", padding_mode="zeros",
                         align_corners=False).permute(0, 2, 3, 1)
    close(got.detach(), want.detach().contiguous())
    (got * dout).sum().backward()
    (want * dout).sum().backward()
    keep = NR.sample_grad_keep(src.detach(), H, W)
    assert float((~keep).double().mean()) < 0.01 or src.numel() < 200
    top = max(float(s2.grad.abs().max()), 1e-300)
    assert float((src.grad - s2.grad)[keep].abs().max()) <= LIMIT * top
    # outside [0, 1] the clamp stops the gradient; on 0 and 1 it passes
    out = (src.detach() < 0) | (src.detach() > 1)
    assert bool((src.grad[out] == 0).all())


def test_sample_grad_keep_leaves_out_the_jumps_and_keeps_the_corners():
    H, W = 4, 8
    src = torch.tensor([[[0.0, 1.0], [0.5 / W, 0.3], [0.3, 1.5 / H], [1e-7, 0.3], [0.3, 1.0 - 1e-7], [0.3, 0.4], [-0.1, 1.1]]])
    assert NR.sample_grad_keep(src, H, W).tolist() == [[True, False, False, False, False, True, True]]


def test_error_bar_and_mask_share():
    r64 = torch.tensor([1.0, -2.0], dtype=D)
    unit, b = NR.bar(r64, torch.tensor([1.0, -2.0 + 1e-6]).float(), 5)
    assert abs(unit - abs(float(torch.tensor(-2.0 + 1e-6).float()) + 2.0)) < 1e-15 and abs(b - (4 * unit + 5 * NR.EPS32 * 2.0)) < 1e-18
    assert NR.judge("c", "x", r64.float(), r64, r64.float(), 1) is None
    assert NR.judge("c", "x", torch.tensor([1.0, -2.001]), r64, r64.float(), 1) is not None
    assert NR.judge("c", "x", torch.tensor([1.0, float("nan")]), r64, r64.float(), 1) is not None
    assert NR.judge("c", "x", r64.float(), r64, (r64 * 1.01).float(), 1) is not None          # a bar looser than the earlier tolerance
    gen = torch.Generator().manual_seed(0)
    m = (torch.rand(100000, generator=gen) >= 0.1).float()
    assert NR.zero_share_ok(m, 0.1)[0] and not NR.zero_share_ok(m, 0.12)[0]
