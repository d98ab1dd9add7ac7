"""TEST INFRASTRUCTURE: dtype-generic specifications of the first-generation operators (csrc/norm.hip, csrc/attn.hip, csrc/tps.hip).
Plain torch with every formula written out, so that one function is the float64 reference and, run in float32 on the CPU, the unit of
the error bars.  tests/test_norm_attn_ref.py pins each of them on the CPU against torch's own float64 operator and against float64
autograd; the GPU files tests/test_{norm,attn,tps}_routes_gpu.py compare the HIP kernels with them.

Dropout: the kernels draw keep bits from (seed word, site, flat index).  The specifications take the scaled keep mask (0 or 1 / (1 - p))
as an INPUT; `recover_mask` obtains it from tatt_dropout over a tensor of ones, whose flat index is that of the contiguous tensor.

Error bars (`bar`, `judge`): 4 x unit + k x EPS32 x max|reference|; unit = max-abs distance of the float32 CPU run of the specification
from its float64 run on the same inputs and mask, k = fp32 roundings on the kernel's longest dependent chain for that output (stated
next to each operator in the GPU files).  A bar is never looser than the tolerance the operator was tested with before.
"""
import math

import torch

EPS32 = float(torch.finfo(torch.float32).eps)
ACT_NONE, ACT_RELU, ACT_MISH = 0, 1, 2
HEADS, HEAD_DIM = 4, 16


# ---- activations ---------------------------------------------------------------------------------------------------------------------
def act_fn(u, act):
    if act == ACT_RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == ACT_MISH:                                       # u tanh(softplus(u)), softplus = identity beyond 20
        sp = torch.where(u > 20.0, u, torch.log1p(torch.exp(torch.clamp(u, max=20.0))))
        return u * torch.tanh(sp)
    assert act == ACT_NONE
    return u


def act_grad(u, act):
    if act == ACT_RELU:
        return (u > 0).to(u.dtype)
    if act == ACT_MISH:                                       # tanh(sp) + u (1 - tanh(sp)^2) sigmoid(u); softplus' = 1 beyond 20
        sp = torch.where(u > 20.0, u, torch.log1p(torch.exp(torch.clamp(u, max=20.0))))
        t = torch.tanh(sp)
        sg = torch.where(u > 20.0, torch.ones_like(u), 1.0 / (1.0 + torch.exp(-u)))
        return t + u * (1.0 - t * t) * sg
    assert act == ACT_NONE
    return torch.ones_like(u)


# ---- BatchNorm over the rows of (M, C) ---------------------------------------------------------------------------------------------
def bn_forward(x, gamma, beta, running_mean, running_var, training, momentum, eps, act):
    """-> y, mean, rstd, new_running_mean, new_running_var.  train: batch mean and BIASED variance normalise, the running variance takes
    the UNBIASED one (M > 1); eval: the running statistics normalise and stay."""
    M = x.shape[0]
    if training:
        mean = x.sum(0) / M
        var = ((x - mean) ** 2).sum(0) / M
        unb = var * (M / (M - 1.0)) if M > 1 else var
        new_rm = (1.0 - momentum) * running_mean + momentum * mean
        new_rv = (1.0 - momentum) * running_var + momentum * unb
    else:
        mean, var, new_rm, new_rv = running_mean, running_var, running_mean, running_var
    rstd = 1.0 / torch.sqrt(var + eps)
    y = act_fn((x - mean) * rstd * gamma + beta, act)
    return y, mean, rstd, new_rm, new_rv


def bn_partial_sums(x, dy, mean, rstd, gamma, beta, act):
    """-> du, xhat, sum du, sum du xhat   (du = dy act'(gamma xhat + beta))"""
    xh = (x - mean) * rstd
    du = dy * act_grad(gamma * xh + beta, act)
    return du, xh, du.sum(0), (du * xh).sum(0)


def bn_backward(x, dy, mean, rstd, gamma, beta, act, training):
    """-> dx, dgamma, dbeta"""
    M = x.shape[0]
    du, xh, s, q = bn_partial_sums(x, dy, mean, rstd, gamma, beta, act)
    v = du - s / M - xh * (q / M) if training else du
    return gamma * rstd * v, q, s


def bn_backward_finish(s, q, M, mean, rstd, gamma):
    """the sums of `bn_partial_sums` -> dgamma, dbeta, coef (3, C) with  dx = coef[0] du + coef[1] x + coef[2]  (train mode)"""
    a = gamma * rstd
    b = -a * rstd * (q / M)
    c = -a * (s / M) - b * mean
    return q, s, torch.stack([a, b, c])


def bn_backward_affine(x, du, coef):
    return coef[0] * du + coef[1] * x + coef[2]


# ---- LayerNorm over the last axis with a residual ----------------------------------------------------------------------------------
def _ln_parts(a, b, eps, mode, mask):
    x = a if b is None else a + (b if mask is None else b * mask)
    C = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / C
    ssq = ((x - mu) ** 2).sum(-1, keepdim=True)
    if mode == 0:                                             # nn.LayerNorm
        rs = 1.0 / torch.sqrt(ssq / C + eps)
    else:                                                     # TBSRN: unbiased std, eps outside the root
        assert mode == 1 and C >= 2
        rs = 1.0 / (torch.sqrt(ssq / (C - 1)) + eps)
    return (x - mu) * rs, rs


def layer_norm(a, b, gamma, beta, eps, mode, mask):
    xh, _ = _ln_parts(a, b, eps, mode, mask)
    return xh * gamma + beta


def layer_norm_backward(a, b, dy, gamma, eps, mode, mask):
    """-> dx (gradient of a), db (of b in front of its dropout; None without b), dgamma, dbeta"""
    xh, rs = _ln_parts(a, b, eps, mode, mask)
    C = a.shape[-1]
    g = dy * gamma
    s1 = g.sum(-1, keepdim=True) / C
    s2 = (g * xh).sum(-1, keepdim=True)
    if mode == 0:
        dx = rs * (g - s1 - xh * (s2 / C))
    else:
        std = 1.0 / rs - eps
        dx = rs * (g - s1) - xh * (s2 / ((C - 1) * std))
    db = None if b is None else (dx if mask is None else dx * mask)
    red = tuple(range(a.dim() - 1))
    return dx, db, (dy * xh).sum(red), dy.sum(red)


# ---- attention core: 4 heads of 16, Q already scaled -------------------------------------------------------------------------------
def attn_core(Q, K, V, mask):
    """Q (B, Lq, 64), K, V (B, S, 64), mask (B, 4, Lq, S) or None -> ctx (B, Lq, 64), wavg (B, Lq, S) = head mean of the dropped
    probabilities"""
    B, Lq, E = Q.shape
    S = K.shape[1]
    assert E == HEADS * HEAD_DIM
    q = Q.reshape(B, Lq, HEADS, HEAD_DIM).permute(0, 2, 1, 3)
    k = K.reshape(B, S, HEADS, HEAD_DIM).permute(0, 2, 1, 3)
    v = V.reshape(B, S, HEADS, HEAD_DIM).permute(0, 2, 1, 3)
    sc = q @ k.transpose(-1, -2)                              # (B, 4, Lq, S)
    e = torch.exp(sc - sc.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    pd = p if mask is None else p * mask
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B, Lq, E)
    return ctx, pd.sum(1) / HEADS


# ---- row softmax ---------------------------------------------------------------------------------------------------------------------
def softmax_rows(S, mask):
    """-> P, Pd = P mask"""
    e = torch.exp(S - S.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    return p, (p if mask is None else p * mask)


# ---- thin-plate-spline grid and bilinear sampling ----------------------------------------------------------------------------------
def tps_grid(ctrl, inv, pad, repr_):
    """ctrl (B, N, 2), inv (N+3, N+3), pad (3, 2), repr (P, N+3) -> (B, P, 2) = repr @ (inv @ cat(ctrl, pad))"""
    B = ctrl.shape[0]
    Y = torch.cat([ctrl, pad.unsqueeze(0).expand(B, 3, 2)], 1)
    return repr_ @ (inv @ Y)


def pixel_coords(src, H, W):
    """the pixel coordinates (ix, iy) that `grid_sample_nhwc` interpolates at"""
    c = torch.clamp(src, 0.0, 1.0)
    gx, gy = 2.0 * c[..., 0] - 1.0, 2.0 * c[..., 1] - 1.0
    return ((gx + 1.0) * W - 1.0) * 0.5, ((gy + 1.0) * H - 1.0) * 0.5


def grid_sample_nhwc(x, src):
    """x (B, C, H, W), src (B, H*W, 2) -> (B, H, W, C): bilinear, zeros outside, align_corners=False, at 2 clamp(src, 0, 1) - 1"""
    B, C, H, W = x.shape
    ix, iy = pixel_coords(src, H, W)                          # (B, H*W)
    fx, fy = torch.floor(ix), torch.floor(iy)
    tx, ty = ix - fx, iy - fy
    x0, y0 = fx.long(), fy.long()
    flat = x.reshape(B, C, H * W)

    def tap(yi, xi):
        inside = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).to(x.dtype)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).unsqueeze(1).expand(B, C, H * W)
        return flat.gather(2, idx) * inside.unsqueeze(1)

    out = (tap(y0, x0) * ((1.0 - tx) * (1.0 - ty)).unsqueeze(1) + tap(y0, x0 + 1) * (tx * (1.0 - ty)).unsqueeze(1)
           + tap(y0 + 1, x0) * ((1.0 - tx) * ty).unsqueeze(1) + tap(y0 + 1, x0 + 1) * (tx * ty).unsqueeze(1))
    return out.reshape(B, C, H, W).permute(0, 2, 3, 1)


def sample_grad_keep(src, H, W):
    """the points whose d out / d src is compared: not within 1e-4 of an integer pixel coordinate (the derivative jumps there), not
    within 1e-6 of the clamp's corners 0 and 1 without lying on them (on them both sides pass the gradient)"""
    s = src.double()
    ix, iy = pixel_coords(s, H, W)
    near_int = ((ix - torch.round(ix)).abs() < 1e-4) | ((iy - torch.round(iy)).abs() < 1e-4)
    near_edge = torch.zeros_like(near_int)
    for e in (0.0, 1.0):
        near_edge |= (((s - e).abs() < 1e-6) & (s != e)).any(-1)
    return ~(near_int | near_edge)


def sample_inputs(B, C, H, W, seed):
    """x (B, C, H, W), src (B, H*W, 2) uniform on [-0.2, 1.2] with some entries exactly 0 and exactly 1, dout (B, H, W, C)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen)
    src = torch.rand(B, H * W, 2, generator=gen) * 1.4 - 0.2
    flat = src.view(-1)
    n = flat.numel()
    every7 = torch.arange(0, n + 7, 7)
    flat[every7[every7 < n][:max(1, n // 14)]] = 0.0
    flat[(every7 + 3)[every7 + 3 < n][:max(1, n // 14)]] = 1.0
    if n == 2:                                               # (one point: x on the corner 0, y inside)
        flat[1] = 0.3
    dout = torch.randn(B, H, W, C, generator=gen)
    return x, src, dout


# ---- dropout masks -------------------------------------------------------------------------------------------------------------------
def zero_share_ok(mask, p):
    """the share of zeros of a keep mask lies within p +- 5 sqrt(p (1 - p) / n)"""
    n = mask.numel()
    share = float((mask == 0).double().mean())
    return abs(share - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), share


def recover_mask(shape, p, seed, site, dev):
    """the scaled keep mask (0 or 1 / (1 - p), on the CPU) the kernels draw for a contiguous tensor of `shape`: tatt_dropout over ones"""
    from tatt_amd import ops
    m = ops.dropout(torch.ones(shape, device=dev), p, seed, site).cpu()
    keep = m != 0
    if bool(keep.any()):
        assert bool((m[keep] == m[keep][0]).all()) and abs(float(m[keep][0]) - 1.0 / (1.0 - p)) <= 2 * EPS32 / (1.0 - p)
    ok, share = zero_share_ok(m, p)
    assert ok, (share, p, m.numel())
    return m


# ---- buffers with canaries -----------------------------------------------------------------------------------------------------------
LAYOUTS = {"contig": (0, 0), "slice16": (8, 4), "off1": (3, 1)}       # name -> (extra columns of the wider map, column offset of the slice)
PAD = 8                                                                # canary elements in front of and behind a map (32 bytes)


class Box:
    """A device buffer of canaries (tests/step_tail_ref.py) with a view `v` inside it: an (M, C) map -- contiguous, a 16-byte aligned
    column slice of a wider map or a slice at column offset 1 -- or a vector at element offset 4 (16-byte aligned) or 5.  Given values,
    the view holds them (an input: whatever a kernel reads outside it is a NaN); `intact()`: nothing outside the view changed."""

    def __init__(self, buf0, lo, M, ld, off, C, dev):
        from tests.step_tail_ref import bits
        self._bits = bits
        self.buf0 = buf0
        self.buf = buf0.to(dev)
        self.v = self.buf[lo:lo + M * ld].view(M, ld)[:, off:off + C]
        inside = torch.zeros(buf0.numel(), dtype=torch.bool)
        inside[lo:lo + M * ld].view(M, ld)[:, off:off + C] = True
        self.outside = ~inside
        assert self.buf.data_ptr() % 16 == 0

    def intact(self):
        return bool(torch.equal(self._bits(self.buf)[self.outside], self._bits(self.buf0)[self.outside]))


def box2d(t, M, C, layout, dev):
    from tests.step_tail_ref import canary
    extra, off = LAYOUTS[layout]
    ld = C + extra
    buf0 = canary(PAD + M * ld + PAD).clone()
    if t is not None:
        buf0[PAD:PAD + M * ld].view(M, ld)[:, off:off + C] = t.reshape(M, C)
    b = Box(buf0, PAD, M, ld, off, C, dev)
    assert b.v.stride() == (ld, 1) and (b.v.data_ptr() % 16 == 0) == (off % 4 == 0)
    return b


def boxvec(t, n, odd, dev):
    from tests.step_tail_ref import canary
    lead = 5 if odd else 4
    buf0 = canary(lead + n + 4).clone()
    if t is not None:
        buf0[lead:lead + n] = t.reshape(-1)
    b = Box(buf0, lead, 1, n, 0, n, dev)
    b.v = b.v.reshape(n)
    assert (b.v.data_ptr() % 16 == 0) == (not odd)
    return b


# ---- error bars ----------------------------------------------------------------------------------------------------------------------
def bar(ref64, ref32, k):
    """-> unit, bar"""
    unit = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    top = float(ref64.abs().max()) if ref64.numel() else 0.0
    return unit, 4.0 * unit + k * EPS32 * top


def legacy_bound(ref64, grad, rtol=None, atol=None):
    """what compare_fn allowed at the largest element (rtol 2e-4 / atol 2e-5 on values, 5e-4 / 5e-5 max(1, max|g|) on gradients)"""
    top = float(ref64.abs().max()) if ref64.numel() else 0.0
    if grad:
        rtol, atol = (5e-4 if rtol is None else rtol), (5e-5 if atol is None else atol) * max(1.0, top)
    else:
        rtol, atol = (2e-4 if rtol is None else rtol), (2e-5 if atol is None else atol)
    return atol + rtol * top


def judge(case, name, got, ref64, ref32, k, grad=False, keep=None, legacy=None):
    """print case, unit, bar, error; -> None or the failure.  keep: boolean mask of the compared elements"""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (case, name, tuple(got.shape), tuple(ref64.shape))
    if keep is not None:
        got, ref64, ref32 = got[keep], ref64[keep], ref32[keep]
    unit, b = bar(ref64, ref32, k)
    err = float((got - ref64).abs().max()) if got.numel() else 0.0
    print("%s %-8s unit %.3e  bar %.3e  error %.3e" % (case, name, unit, b, err))
    old = legacy_bound(ref64, grad) if legacy is None else legacy_bound(ref64, grad, *legacy)
    if not b <= old:
        return (case, name, "bar %.3e looser than the earlier tolerance %.3e" % (b, old))
    if not err <= b:                                          # (also catches a NaN)
        return (case, name, "error %.3e above bar %.3e (unit %.3e)" % (err, b, unit))
    return None
