"""The thin-plate-spline grid (tatt_tps_grid_*) and the bilinear sampler (tatt_grid_sample_*) of csrc/tps.hip against the float64
specifications of tests/norm_attn_ref.py, beyond the one golden case (16 x 64, 20 control points, batch 3) of test_tps_golden_and_grad.

Grid, two families:
  * the module's own buffers (TPSSpatialTransformer, 20 control points) at output sizes (16, 64), (32, 128), (64, 256) through
    functional.TpsGridFn -- P = 16384 makes the backward's per-thread sums 64 terms long.  The module's inverse kernel is ill-conditioned
    (entries up to 87 that cancel), so the float32 unit is large there; its bar is capped by the tolerances of test_tps_golden_and_grad;
  * random inv / pad / repr matrices (the kernel is two matrix products) through tatt_amd.ops into canaried buffers, N + 3 up to the limit
    of 32 and P below, at and above one work-group of 256.
Sampler: C = 1, 3, 4 channels, sizes down to one pixel, the image as NCHW, as channels-last and as a channel slice of a wider image,
coordinates on [-0.2, 1.2] (the clamp and its gradient mask) with some exactly 0 and exactly 1.  The gradient is compared away from the
points where it jumps (NR.sample_grad_keep: an integer pixel coordinate, the corners of the clamp), below 1 % of the points.

Error bars: NR.judge, 4 x unit + k x EPS32 x max|reference|; k = fp32 roundings on the longest dependent chain:
  grid      src     2              both products accumulate in fp64 from fp32 operands: the result is rounded once
            dctrl   P / 256 + 2    tps_grid_bwd_kernel: a thread's fp32 chain of fused multiply-adds over its share of the P points, then fp64
  sampler   out     13             the pixel coordinate (5), its fraction, the weights (2), four products and three sums
            dsrc    15 + 2 C       the coordinate and the fraction (6), tap differences and weights (3), 2 C accumulations, the three
                                   factors (0.5 W, 2, the mask: 2 roundings), the sum of the two terms

Measured on the MI355X (unit / bar / error):
  grid, module buffers 16x64       src 4.518e-06 / 1.833e-05 / 5.929e-08   dctrl 6.376e-04 / 2.560e-03 / 5.375e-05
  grid, module buffers 32x128      src 2.622e-06 / 1.074e-05 / 5.956e-08   dctrl 4.312e-03 / 1.730e-02 / 1.764e-04
  grid, module buffers 64x256      src 3.036e-06 / 1.240e-05 / 5.952e-08   dctrl 1.225e-02 / 4.946e-02 / 6.826e-04   (max |dctrl| 59)
  grid, random N=29 P=257          dctrl 2.636e-06 / 1.531e-05 / 5.803e-07
  grid, random N=29 P=1024         src 4.004e-07 / 2.064e-06 / 5.949e-08   dctrl 1.083e-05 / 5.638e-05 / 8.608e-07
  sampler C=3 16x64 B=3 (slice)    out 4.277e-06 / 2.108e-05 / 4.038e-06   dsrc 2.462e-04 / 2.800e-03 / 2.462e-04
  sampler C=1 16x64 B=3 (slice)    out 3.120e-06 / 1.549e-05 / 3.180e-06   dsrc 1.263e-04 / 1.545e-03 / 1.195e-04
  sampler C=3 1x1 B=1              out 2.238e-09 / 3.961e-07 / 2.238e-09   dsrc 1.015e-08 / 1.033e-06 / 1.015e-08
  (the kernels' fp64 accumulation shows: the grid is 10 to 70 times closer to float64 than the float32 specification)
What this file found: no wrong value -- all 46 tests pass on the kernels as they were; the three image layouts give the same bits.
"""
import pytest
import torch

from tests import norm_attn_ref as NR

pytestmark = pytest.mark.gpu
TPS_MAXNP = 32
TPS_LEGACY = {False: (1e-3, 2e-3), True: (1e-2, 1e-2)}   # (rtol, atol) of test_tps_golden_and_grad: values, gradients


def _k_grid(name, P):
    return 2 if name == "src" else -(-P // 256) + 2


def _grid_reference(ctrl, inv, pad, rep, dsrc):
    out = {}
    for dt in (torch.float64, torch.float32):
        c = ctrl.to(dt).clone().requires_grad_()
        src = NR.tps_grid(c, inv.to(dt), pad.to(dt), rep.to(dt))
        (g,) = torch.autograd.grad((src * dsrc.to(dt)).sum(), c)
        out[dt] = {"src": src.detach(), "dctrl": g}
    return out[torch.float64], out[torch.float32]


# ---- the module's buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 64), (32, 128), (64, 256)])
def test_tps_grid_with_the_modules_buffers(dev, size):
    from tatt_amd import functional as Fh
    from tatt_amd.tsrn import TPSSpatialTransformer
    tps = TPSSpatialTransformer(size, 20, (0.05, 0.05))
    B, P = 3, size[0] * size[1]
    gen = torch.Generator().manual_seed(size[0])
    ctrl = tps.target_control_points.unsqueeze(0) + 0.03 * torch.randn(B, 20, 2, generator=gen)
    dsrc = torch.randn(B, P, 2, generator=gen)
    inv, pad, rep = tps.inverse_kernel, tps.padding_matrix, tps.target_coordinate_repr
    assert tuple(rep.shape) == (P, 23) and tuple(inv.shape) == (23, 23) and inv.is_contiguous()
    r64, r32 = _grid_reference(ctrl, inv, pad, rep, dsrc)
    c = ctrl.to(dev).requires_grad_()
    src = Fh.TpsGridFn.apply(c, inv.to(dev), pad.to(dev), rep.to(dev))
    src.backward(dsrc.to(dev))
    tag = "tps grid module %dx%d" % size
    failed = [f for f in (NR.judge(tag, "src", src, r64["src"], r32["src"], _k_grid("src", P), legacy=TPS_LEGACY[False]),
                          NR.judge(tag, "dctrl", c.grad, r64["dctrl"], r32["dctrl"], _k_grid("dctrl", P), grad=True,
                                   legacy=TPS_LEGACY[True])) if f]
    assert not failed, failed


# ---- random matrices ---------------------------------------------------------------------------------------------------------------
GRID_CASES = [(N, P) for N in (1, 20, 28, 29) for P in (1, 35, 255, 256, 257, 1024)]


def _check_grid_cases():
    rows = [{"N + 3 at the limit": N + 3 == TPS_MAXNP, "more than one block of points": P > 256, "a ragged block": P % 256 != 0,
             "threads without a point": P < 256, "one control point": N == 1} for N, P in GRID_CASES]
    for name in rows[0]:
        assert {r[name] for r in rows} == {True, False}, name


_check_grid_cases()


@pytest.mark.parametrize("N,P", GRID_CASES)
def test_tps_grid_random_matrices_against_float64(dev, N, P):
    from tatt_amd import ops
    B, NP = 3, N + 3
    gen = torch.Generator().manual_seed(40 * N + P)
    ctrl, pad = torch.rand(B, N, 2, generator=gen), torch.randn(3, 2, generator=gen)
    inv, rep = torch.randn(NP, NP, generator=gen) / NP ** 0.5, torch.randn(P, NP, generator=gen) / NP ** 0.5
    dsrc = torch.randn(B, P, 2, generator=gen)
    r64, r32 = _grid_reference(ctrl, inv, pad, rep, dsrc)
    cd, invd, padd, repd, dsd = (t.to(dev) for t in (ctrl, inv, pad, rep, dsrc))
    sb, gb = NR.box2d(None, 1, B * P * 2, "contig", dev), NR.box2d(None, 1, B * N * 2, "contig", dev)
    ops.call("tatt_tps_grid_fwd", ops.P(cd), ops.P(invd), ops.P(padd), ops.P(repd), ops.P(sb.v), B, N, P, ops.stream())
    ops.call("tatt_tps_grid_bwd", ops.P(dsd), ops.P(invd), ops.P(repd), ops.P(gb.v), B, N, P, ops.stream())
    src, dctrl = sb.v.reshape(B, P, 2), gb.v.reshape(B, N, 2)
    assert torch.equal(ops.tps_grid_fwd(cd, invd, padd, repd), src) and torch.equal(ops.tps_grid_bwd(dsd, invd, repd, N), dctrl)
    tag = "tps grid N=%d P=%d" % (N, P)
    failed = [f for f in (NR.judge(tag, "src", src, r64["src"], r32["src"], _k_grid("src", P)),
                          NR.judge(tag, "dctrl", dctrl, r64["dctrl"], r32["dctrl"], _k_grid("dctrl", P), grad=True)) if f]
    if not (sb.intact() and gb.intact()):
        failed.append((tag, "a canary changed"))
    assert not failed, failed


def test_tps_grid_refuses_30_control_points(dev):
    from tatt_amd import ops
    N, P = 30, 5
    ctrl, inv, rep = torch.rand(1, N, 2, device=dev), torch.randn(N + 3, N + 3, device=dev), torch.randn(P, N + 3, device=dev)
    with pytest.raises(RuntimeError, match="tatt_tps_grid_fwd failed with code 1"):
        ops.tps_grid_fwd(ctrl, inv, torch.zeros(3, 2, device=dev), rep)
    with pytest.raises(RuntimeError, match="tatt_tps_grid_bwd failed with code 1"):
        ops.tps_grid_bwd(torch.randn(1, P, 2, device=dev), inv, rep, N)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(C, H, W, B) for C in (1, 3, 4) for H, W in ((1, 1), (5, 7), (16, 64)) for B in (1, 3)]
IMAGE_LAYOUTS = ("nchw", "channels_last", "channel_slice")


def _sample_seed(C, H, W, B):
    return 1000 * C + H * W + B


def _check_sample_cases():
    """the share of points left out of the gradient comparison, from the reference alone (no GPU): below 1 % wherever there are enough
    points for a share to mean something; a handful of points leaves none out"""
    for C, H, W, B in SAMPLE_CASES:
        x, src, dout = NR.sample_inputs(B, C, H, W, _sample_seed(C, H, W, B))
        keep = NR.sample_grad_keep(src, H, W)
        left_out = int((~keep).sum())
        assert left_out == 0 if keep.numel() < 200 else left_out < 0.01 * keep.numel(), (C, H, W, B, left_out)
        s = src.reshape(-1)
        assert bool((s == 0).any()) and (s.numel() < 4 or bool((s == 1).any()))
        if s.numel() >= 200:
            assert float(s.min()) < -0.1 and float(s.max()) > 1.1 and bool(keep.reshape(-1, 1).expand(-1, 2).reshape(-1)[s == 0].all())
    rows = [{"one pixel": H * W == 1, "more than one block of points": B * H * W > 256, "four channels": C == 4, "one channel": C == 1}
            for C, H, W, B in SAMPLE_CASES]
    for name in rows[0]:
        assert {r[name] for r in rows} == {True, False}, name


_check_sample_cases()


def _image(x, layout, dev):
    """the image on the device as (B, C, H, W) with the strides of `layout`; the channels a slice leaves out hold NaNs"""
    B, C, H, W = x.shape
    xd = x.to(dev)
    if layout == "nchw":
        return xd
    if layout == "channels_last":
        v = xd.contiguous(memory_format=torch.channels_last) if C > 1 else xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert C == 1 or (v.stride(1) == 1 and (H * W == 1 or v.stride(3) == C))
        return v
    wide = torch.full((B, C + 1, H, W), float("nan"), device=dev)
    wide[:, :C] = xd
    v = wide[:, :C]
    assert v.stride(0) == (C + 1) * H * W and v.data_ptr() == wide.data_ptr()
    return v


@pytest.mark.parametrize("C,H,W,B", SAMPLE_CASES)
def test_grid_sample_against_float64(dev, C, H, W, B):
    from tatt_amd import functional as Fh
    from tatt_amd import ops
    x, src, dout = NR.sample_inputs(B, C, H, W, _sample_seed(C, H, W, B))
    keep = NR.sample_grad_keep(src, H, W).unsqueeze(-1).expand(B, H * W, 2)
    ref = {}
    for dt in (torch.float64, torch.float32):
        s = src.to(dt).clone().requires_grad_()
        out = NR.grid_sample_nhwc(x.to(dt), s)
        (g,) = torch.autograd.grad((out * dout.to(dt)).sum(), s)
        ref[dt] = {"out": out.detach(), "dsrc": g}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    outside = (src < 0) | (src > 1)
    assert bool((r64["dsrc"][outside] == 0).all()) and (src.numel() < 200 or float(outside.float().mean()) > 0.1)
    srcd, doutd = src.to(dev), dout.to(dev)
    failed, first = [], None
    for layout in IMAGE_LAYOUTS:
        xd = _image(x, layout, dev)
        tag = "sample C=%d %dx%d B=%d %s" % (C, H, W, B, layout)
        ob, gb = NR.box2d(None, 1, B * H * W * C, "contig", dev), NR.box2d(None, 1, B * H * W * 2, "contig", dev)
        st = xd.stride()
        ops.call("tatt_grid_sample_fwd", ops.P(xd), st[0], st[1], st[2], st[3], ops.P(srcd), ops.P(ob.v), B, C, H, W, ops.stream())
        ops.call("tatt_grid_sample_bwd", ops.P(xd), st[0], st[1], st[2], st[3], ops.P(srcd), ops.P(doutd), ops.P(gb.v), B, C, H, W, ops.stream())
        out, dsrc = ob.v.reshape(B, H, W, C), gb.v.reshape(B, H * W, 2)
        failed.append(NR.judge(tag, "out", out, r64["out"], r32["out"], 13))
        failed.append(NR.judge(tag, "dsrc", dsrc, r64["dsrc"], r32["dsrc"], 15 + 2 * C, grad=True, keep=keep))
        if not bool((dsrc[outside.to(dev)] == 0).all()):
            failed.append((tag, "a gradient passed the clamp"))
        if not (ob.intact() and gb.intact()):
            failed.append((tag, "a canary changed"))
        if first is None:
            first = (out.clone(), dsrc.clone())
        elif not (torch.equal(out, first[0]) and torch.equal(dsrc, first[1])):
            failed.append((tag, "the result depends on the image's strides"))
    # the autograd wiring, once
    s = srcd.clone().requires_grad_()
    o = Fh.GridSampleFn.apply(_image(x, "nchw", dev), s)
    o.backward(doutd)
    if not (torch.equal(o, first[0]) and torch.equal(s.grad, first[1])):
        failed.append(("GridSampleFn", "differs from the direct calls"))
    failed = [f for f in failed if f]
    assert not failed, failed[:8]
