"""The ASTER recogniser's front and encoder against float64 at every route the evaluation loop can take, beyond the one recorded
fixture (three images, batch 3) of tests/test_aster_gpu.py:

  1. every distinct convolution geometry of ResNet_ASTER and of the STN head as ASTER uses it -- walked from the modules, not listed --
     as ONE layer through `ops.conv2d_forward`, filter and bias from `infer.bn_fold`, the input the view the model hands over
     (`h[:, ::sh, ::sw, :]` of a dense NHWC map, the NHWC view of an NCHW image for the head's first layer), on both sides of the batch
     size at which `ops.conv_split` stops splitting the contraction;
  2. the whole front and encoder at batch 1, 2 and 5, as shipped (every deep convolution splits) and with CONV_SPLIT_TILES = 0 (none
     does: the configuration of batch >= 82, at a size that costs nothing);
  3. `resize_bilinear_ac`, `grid_sample_sized` and two stacked `bilstm_eval` layers at the recogniser's sizes and at their edges.

Oracles: tests/aster_ref.py (pinned on the CPU by tests/test_aster.py against what the reference recorded) and torch's float64 operators.
Error bars of 2. and 3.: 4 x the distance of the same oracle run in float32 on the CPU from its float64 run on the same inputs, measured
inside the test, + 1e-7 x the largest value -- the rule of tests/test_aster_gpu.py.  The single layers use `check_close` at the
tolerances of test_conv2d_fn (rtol 2e-4, atol 2e-5, weights scaled by 1 / sqrt(Cin k k)).

Measured on the MI355X (unit = float32 CPU restatement against float64, bar = 4 x unit + 1e-7 x max, error = GPU against float64):
  batch  stage                 unit       bar        error as shipped   error with CONV_SPLIT_TILES = 0
  1      control_points        9.896e-08  4.997e-07  7.570e-08          9.216e-08
  1      rectify               4.677e-04  1.871e-03  1.360e-05          1.678e-05
  1      encode(oracle rect)   8.078e-07  3.280e-06  6.799e-07          9.381e-07
  1      features              2.507e-05  1.003e-04  1.198e-06          1.357e-06
  2      control_points        8.778e-08  4.549e-07  8.455e-08          1.024e-07
  2      rectify               7.662e-04  3.065e-03  1.066e-05          1.180e-05
  2      encode(oracle rect)   8.508e-07  3.453e-06  1.190e-06          2.291e-06
  2      features              3.430e-05  1.372e-04  9.261e-07          2.528e-06
  5      control_points        1.051e-07  5.243e-07  9.790e-08          1.170e-07
  5      rectify               6.368e-04  2.547e-03  1.865e-05          1.580e-05
  5      encode(oracle rect)   1.479e-06  5.968e-06  1.425e-06          1.479e-06
  5      features              7.613e-05  3.046e-04  2.136e-06          1.999e-06
  resize_bilinear_ac (worst of batch 1 and 5, both layouts equal):  (32,128)->(32,64) unit 1.432e-05 bar 5.740e-05 error 7.228e-06;
      (16,64)->(32,64) 1.306e-06 / 5.326e-06 / 8.585e-07;  (5,7)->(3,11) 5.007e-07 / 2.102e-06 / 3.636e-07;  (4,4)->(1,1) and (1,9)->(2,5) exact
  grid_sample_sized:  (32,128)->(32,100) C=3 unit 8.264e-08 bar 4.305e-07 error 1.296e-07, C=4 9.159e-08 / 4.660e-07 / 1.026e-07;
      (8,16)->(3,5) C=3 3.755e-08 / 2.390e-07 / 3.755e-08, C=4 5.086e-08 / 3.001e-07 / 6.300e-08
  two BiLSTM layers, I = 512, T = 25:  B=1 3.015e-07, B=5 3.610e-07, B=129 (per-step kernels) 4.695e-07 (limit 1e-5)
The rectified image's unit is large because the images are noise: a sampling position that the float32 CPU run has off by 1e-6 of
the image width (its `src` stage) is 1e-4 of a pixel, between neighbours that differ by up to 2.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tatt_amd
from tatt_amd import aster, infer, ops
from tatt_amd._lib import LIB
from tatt_amd.ops import ACT_NONE, ACT_RELU
from tatt_amd.tsrn import STNHead

import aster_ref as R
from tests.util import check_close, max_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KW = dict(arch="ResNet_ASTER", rec_num_classes=97, sDim=512, attDim=512, max_len_labels=100, eos=94, STN_ON=True)
EPS32 = float(torch.finfo(torch.float32).eps)
BATCH_LIMIT = 256                  # a split boundary above it is reached with CONV_SPLIT_TILES = 0 at batch 3 instead


# ---- 1. single layers ------------------------------------------------------------------------------------------------------------------
def _geometries():
    """{(H, W, Cin, Cout, k, (sh, sw), act, nchw): first layer of that geometry}: H x W is the map the convolution runs on (the
    sub-sampled view where the layer has a stride), nchw marks the input that is the NHWC view of an NCHW tensor"""
    found = {}

    def add(where, H, W, conv, sub, act, nchw=False):
        k = conv.kernel_size[0]
        assert conv.kernel_size == (k, k) and conv.padding == (k // 2, k // 2) and tuple(conv.stride) == tuple(sub), where
        found.setdefault((H, W, conv.in_channels, conv.out_channels, k, tuple(sub), act, nchw), where)

    with torch.device("meta"):                                         # (shapes only: no 20M parameters are drawn)
        enc = aster.ResNet_ASTER()
    H, W = R.TPS_OUT
    add("layer0", H, W, enc.layer0[0], (1, 1), ACT_RELU)
    for li in range(1, 6):
        for bi, blk in enumerate(getattr(enc, "layer%d" % li)):
            sh, sw = blk.stride
            H, W = len(range(0, H, sh)), len(range(0, W, sw))          # the size of h[:, ::sh, ::sw, :]
            add("layer%d.%d.conv1" % (li, bi), H, W, blk.conv1, (sh, sw), ACT_RELU)
            add("layer%d.%d.conv2" % (li, bi), H, W, blk.conv2, (1, 1), ACT_NONE)
            if blk.downsample is not None:
                add("layer%d.%d.downsample" % (li, bi), H, W, blk.downsample[0], (sh, sw), ACT_NONE)
    assert (H, W) == (1, 25)
    head = STNHead(in_planes=3, num_ctrlpoints=aster.NUM_CONTROL_POINTS, activation="none")
    H, W = R.TPS_IN
    for i in (0, 2, 4, 6, 8, 10):                                      # ASTER.control_points: conv, then a 2 x 2 pool after all but the last
        add("stn%d" % i, H, W, head.stn_convnet[i][0], (1, 1), ACT_RELU, nchw=(i == 0))
        if i != 10:
            H, W = H // 2, W // 2
    assert (H, W) == (1, 2)
    return found


GEOMS = _geometries()


def _gid(g):
    H, W, Cin, Cout, k, (sh, sw), act, nchw = g
    return "%s-%dx%d-%dto%d-k%d-sub%dx%d-%s" % (GEOMS[g], H, W, Cin, Cout, k, sh, sw, "relu" if act == ACT_RELU else "none")


def _splits(g, B):
    H, W, Cin, Cout, k = g[:5]
    return ops.conv_split(torch.empty(B, H, W, Cin, device="meta"), Cout, k, k)


def _boundary(g):
    """None: the geometry never splits; B: the smallest batch that does not split (B - 1 does); BATCH_LIMIT + 1: it splits up to the limit"""
    if _splits(g, 1) == 1:
        assert all(_splits(g, B) == 1 for B in (2, 3, 5, 64, BATCH_LIMIT))
        return None
    for B in range(2, BATCH_LIMIT + 1):
        if _splits(g, B) == 1:
            return B
    return BATCH_LIMIT + 1


def _ragged_batch(H, W):
    """the smallest batch from 4 on with more than one row tile of 64 pixels and a partial last one (None: H * W is a multiple of 64)"""
    for B in range(4, 70):
        if B * H * W > 64 and (B * H * W) % 64:
            return B
    return None


def test_the_walk_finds_the_split_boundaries_of_the_layer_table():
    """the boundaries `conv_split` gives today, recomputed: if a threshold moves, this names the layer"""
    got = {GEOMS[g].split(".")[0] + ":%dx%d:%d->%d:k%d" % (g[0], g[1], g[2], g[3], g[4]): _boundary(g) for g in GEOMS if _boundary(g)}
    print(got)
    want = {"layer2:8x25:64->64:k3": 82, "layer3:4x25:128->128:k3": 82, "layer4:2x25:256->256:k3": 81, "layer5:1x25:512->512:k3": 80,
            "layer5:1x25:512->512:k1": 80, "stn4:8x16:64->128:k3": 64, "stn6:4x8:128->256:k3": 127, "stn8:2x4:256->256:k3": BATCH_LIMIT + 1,
            "stn10:1x2:256->256:k3": BATCH_LIMIT + 1}
    assert got == want
    assert sum(1 for g in GEOMS if g[4] == 1) >= 8 and sum(1 for g in GEOMS if g[3] == 32) >= 4 and sum(1 for g in GEOMS if g[2] == 3) == 2


@pytest.mark.parametrize("g", list(GEOMS), ids=_gid)
def test_conv_geometry_against_float64(dev, g, monkeypatch):
    H, W, Cin, Cout, k, (sh, sw), act, nchw = g
    gen = torch.Generator().manual_seed(1000 * H + 10 * Cin + Cout + k + sh)
    with_bias = GEOMS[g].startswith("stn")                             # the head's convolutions have a bias, the encoder's none
    w = torch.randn(Cout, Cin, k, k, generator=gen) / math.sqrt(Cin * k * k)
    cb = torch.randn(Cout, generator=gen) if with_bias else None
    bn = torch.nn.BatchNorm2d(Cout)
    with torch.no_grad():
        bn.running_mean.copy_(0.3 * torch.randn(Cout, generator=gen))
        bn.running_var.copy_(0.5 + torch.rand(Cout, generator=gen))
        bn.weight.copy_(0.5 + torch.rand(Cout, generator=gen))
        bn.bias.copy_(0.3 * torch.randn(Cout, generator=gen))
    bn_dev = torch.nn.BatchNorm2d(Cout).to(dev).eval()
    bn_dev.load_state_dict(bn.state_dict())
    bn.requires_grad_(False), bn_dev.requires_grad_(False)
    wf, bf = infer.bn_fold(w.to(dev), None if cb is None else cb.to(dev), bn_dev)
    # the fold against torch fp32 on the device (the host's fp32 square root need not be correctly rounded: one CPU gave s 2 ulp off): w s
    # bitwise or to 1 ulp, (b - mean) s + beta to 1 ulp of its larger term (the kernel may contract it)
    s = bn_dev.weight / torch.sqrt(bn_dev.running_var + bn_dev.eps)
    w_want = w.to(dev) * s.view(-1, 1, 1, 1)
    assert bool(((wf - w_want).abs() <= EPS32 * w_want.abs()).all())
    t = (cb.to(dev) if with_bias else torch.zeros(Cout, device=dev)) - bn_dev.running_mean
    b_want = t.double() * s.double() + bn_dev.bias.double()
    assert bool(((bf.double() - b_want).abs() <= EPS32 * ((t * s).abs() + bn_dev.bias.abs()).double()).all())

    bnd = _boundary(g)
    if bnd is None:
        rb = _ragged_batch(H, W)
        plan = [(1, False), (3, False), (rb if rb is not None else 5, False)]
    elif bnd > BATCH_LIMIT:
        plan = [(1, False), (3, False), (3, True)]
    else:
        plan = [(1, False), (3, False), (bnd - 1, False), (bnd, False)]
    fast = Cout % 64 == 0 and Cin % 16 == 0 and not nchw               # (what try_conv_fast takes; the rest runs launch_gemm<3, 16>)
    report, off_side = [], []
    for B, patched in plan:
        if patched:
            monkeypatch.setattr(ops, "CONV_SPLIT_TILES", 0)
        x = torch.randn(B, Cin, H * sh, W * sw, generator=gen)         # the dense map the layer's input is a view of
        xd = x.to(dev)
        if nchw:
            xin = xd.permute(0, 2, 3, 1)
        else:
            dense = xd.permute(0, 2, 3, 1).contiguous()
            xin = dense[:, ::sh, ::sw, :] if (sh, sw) != (1, 1) else dense
        assert tuple(xin.shape) == (B, H, W, Cin)
        splits = ops.conv_split(xin, Cout, k, k)
        report.append("B=%d%s: %d" % (B, " (CONV_SPLIT_TILES=0)" if patched else "", splits))
        want_split = not (bnd is None or patched) and (bnd > BATCH_LIMIT or B < bnd)
        if (splits > 1) != want_split:
            off_side.append((B, patched, splits))
        y = ops.conv2d_forward(xin, wf, bf, act)
        assert tuple(y.shape) == (B, H, W, Cout) and y.is_contiguous()
        ref = F.conv2d(x.double(), w.double(), None if cb is None else cb.double(), stride=(sh, sw), padding=k // 2)
        ref = R.batch_norm_eval(ref, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), bn.eps)
        ref = torch.relu(ref) if act == ACT_RELU else ref
        assert act in (ACT_RELU, ACT_NONE)
        check_close("%s B=%d splits=%d" % (_gid(g), B, splits), y, ref.permute(0, 2, 3, 1), rtol=2e-4, atol=2e-5)
        if act == ACT_NONE and k == 3:                                 # a block's conv2: relu(o + residual) follows it
            res = torch.randn(y.shape, generator=gen).to(dev)
            assert torch.equal(aster.add_relu(y, res), torch.relu(y + res))
    print("%s [%s]%s split counts %s" % (_gid(g), "im2col fast route" if fast else "general route",
                                         "" if bnd is None or bnd > BATCH_LIMIT else " boundary %d | %d" % (bnd - 1, bnd), ", ".join(report)))
    if bnd is None and _ragged_batch(H, W) is None:
        print("    (%d x %d pixels are a multiple of the 64-row tile: no batch leaves a ragged last tile)" % (H, W))
    tatt_amd.sync_check()
    # (asked last, so that a moved threshold still leaves every value compared)
    assert not off_side, "the test no longer straddles the split boundary: (batch, CONV_SPLIT_TILES=0, splits) %s" % off_side


# ---- 2. the whole front and encoder at other batch sizes, split on and off ---------------------------------------------------------
BATCHES = (1, 2, 5)


@pytest.fixture(scope="module")
def world():
    """the fixture's recogniser on the device, and the restatement's float64 and float32 runs on seeded images, computed once for the
    images of all batch sizes (every stage is per image in eval mode) and left unchanged"""
    e2e = np.load(os.path.join(GOLD, "aster_e2e.npz"))
    m = R.e2e_model(tatt_amd.ASTER, **KW)
    with torch.no_grad():                                              # (the recorded inverse, as from a checkpoint: see test_aster_gpu.py)
        m.tps.inverse_kernel.copy_(torch.from_numpy(e2e["tps_inverse_kernel"]))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(29)
    img = torch.rand(sum(BATCHES), 3, 32, 128, generator=g) * 2 - 1
    o64, o32 = R.front(sd, img, torch.float64), R.front(sd, img, torch.float32)
    n = img.shape[0]
    rect_in = o64["rect"].float()                                      # the oracle's own rectified image, as the device receives it
    f64 = R.feats(sd, torch.cat([o64["rect"], rect_in.double()]), torch.float64)
    f32 = R.feats(sd, torch.cat([o32["rect"], rect_in]), torch.float32)
    o64["feats"], o64["feats_at_rect"], o32["feats"], o32["feats_at_rect"] = f64[:n], f64[n:], f32[:n], f32[n:]
    lo, rows = 0, {}
    for B in BATCHES:
        rows[B] = slice(lo, lo + B)
        lo += B
    return {"model": m.to(DEV).eval(), "img": img, "rect_in": rect_in, "o64": o64, "o32": o32, "rows": rows}


@pytest.mark.parametrize("split", ["shipped", "no_split"])
@pytest.mark.parametrize("B", BATCHES)
def test_front_and_encoder_at_batch(world, B, split, monkeypatch):
    deep = [g for g in GEOMS if g[2] * g[4] * g[4] >= 512]             # contractions of 32 chunks of 16 and more
    if split == "no_split":
        monkeypatch.setattr(ops, "CONV_SPLIT_TILES", 0)
    # shipped: every deep convolution splits; with the hook: none does (asserted last, so that a moved threshold still leaves every value compared)
    configured = len(deep) == 9 and all((_splits(g, B) > 1) == (split == "shipped") for g in deep)
    m, rows = world["model"], world["rows"][B]
    img = world["img"][rows].to(DEV)
    with torch.no_grad():
        got = {"ctrl": m.control_points(img), "rect": m.rectify(img).permute(0, 3, 1, 2),
               "feats_at_rect": m.encode(world["rect_in"][rows].to(DEV).permute(0, 2, 3, 1)), "feats": m.features(img)}
    assert tuple(got["feats"].shape) == (B, 25, 512)
    failed = []
    for name, label in (("ctrl", "control_points"), ("rect", "rectify"), ("feats_at_rect", "encode(oracle rect)"), ("feats", "features")):
        want, w32 = world["o64"][name][rows], world["o32"][name][rows]
        unit = float((w32.double() - want).abs().max())
        bar = 4.0 * unit + 1e-7 * float(want.abs().max())
        err = max_err(got[name], want)
        print("B=%d %-8s %-20s unit %.3e  bar %.3e  error %.3e" % (B, split, label, unit, bar, err))
        if not err <= bar:
            failed.append((label, err, bar))
    assert not failed, failed
    tatt_amd.sync_check()
    assert configured, "the deep convolutions do not all %s at batch %d" % ("split" if split == "shipped" else "run unsplit", B)


# ---- 3. the two front kernels and the LSTM at the recogniser's sizes ---------------------------------------------------------------
def _bar(unit_run, want):
    unit = float((unit_run.double() - want).abs().max())
    return unit, 4.0 * unit + 1e-7 * float(want.abs().max())


@pytest.mark.parametrize("src_size,dst_size", [((32, 128), (32, 64)), ((16, 64), (32, 64)), ((5, 7), (3, 11)), ((4, 4), (1, 1)), ((1, 9), (2, 5))])
def test_resize_bilinear_ac_sizes(dev, src_size, dst_size):
    gen = torch.Generator().manual_seed(src_size[0] * 100 + dst_size[1])
    for B in (1, 5):
        four = torch.rand(B, 4, *src_size, generator=gen) * 2 - 1
        x = four[:, :3]
        want = F.interpolate(x.double(), dst_size, mode="bilinear", align_corners=True)
        unit, bar = _bar(F.interpolate(x.contiguous(), dst_size, mode="bilinear", align_corners=True), want)
        fd = four.to(dev)
        for name, xin in (("contiguous", fd[:, :3].contiguous()), ("[:, :3] view", fd[:, :3])):
            got = aster.resize_bilinear_ac(xin, dst_size)
            assert tuple(got.shape) == (B, 3) + dst_size and got.is_contiguous()
            err = max_err(got, want)
            print("resize %s -> %s B=%d %-12s unit %.3e  bar %.3e  error %.3e" % (src_size, dst_size, B, name, unit, bar, err))
            assert err <= bar
    tatt_amd.sync_check()


def _sampling_grid(B, Ho, Wo, H, W, gen):
    """(B, Ho * Wo, 2) fp32 positions: uniform in [-0.3, 1.3] (all four out-of-range sides and the corners), coordinates exactly 0 and
    exactly 1, and coordinates exactly on cell boundaries, (k + 0.5) / W and (k + 0.5) / H (exact in fp32 for these sizes)"""
    src = torch.rand(B, Ho * Wo, 2, generator=gen) * 1.6 - 0.3
    idx = torch.arange(Ho * Wo)
    src[:, idx % 7 == 0, 0] = 0.0
    src[:, idx % 7 == 1, 0] = 1.0
    src[:, idx % 7 == 2, 1] = 0.0
    src[:, idx % 7 == 3, 1] = 1.0
    src[:, idx % 7 == 4, 0] = (((idx * 5) % W).float()[idx % 7 == 4] + 0.5) / W
    src[:, idx % 7 == 5, 1] = (((idx * 3) % H).float()[idx % 7 == 5] + 0.5) / H
    if Ho >= 4:                                                        # whole rows at the corners of the clamp
        rows = src.view(B, Ho, Wo, 2)
        rows[:, Ho - 1] = 0.0
        rows[:, Ho - 2] = 1.0
        rows[:, Ho - 3, :, 0], rows[:, Ho - 3, :, 1] = 0.0, 1.0
        rows[:, Ho - 4, :, 0] = ((torch.arange(Wo) * 9) % W + 0.5) / W
    return src.contiguous()


@pytest.mark.parametrize("src_size,dst_size", [((32, 128), (32, 100)), ((8, 16), (3, 5))])
@pytest.mark.parametrize("C", [3, 4])
def test_grid_sample_sized_edges(dev, src_size, dst_size, C):
    H, W = src_size
    gen = torch.Generator().manual_seed(H + W + C)
    B = 3
    four = torch.rand(B, 4, H, W, generator=gen) * 2 - 1
    src = _sampling_grid(B, dst_size[0], dst_size[1], H, W, gen)
    assert float(src.min()) < -0.2 and float(src.max()) > 1.2 and bool((src == 0).any()) and bool((src == 1).any())
    cell = src[..., 0].double() * W - 0.5
    assert bool(((cell == cell.round()) & (src[..., 0] > 0) & (src[..., 0] < 1)).any())      # positions exactly on a cell boundary
    x = four[:, :C]
    want = R.sample(x, src, dst_size, torch.float64)
    unit, bar = _bar(R.sample(x.contiguous(), src, dst_size, torch.float32), want)
    fd, sd = four.to(dev), src.to(dev)
    layouts = [("contiguous", fd[:, :C].contiguous())] + ([("[:, :3] view", fd[:, :3])] if C == 3 else [])
    for name, xin in layouts:
        got = aster.grid_sample_sized(xin, sd, dst_size).permute(0, 3, 1, 2)
        err = max_err(got, want)
        print("grid_sample %s -> %s C=%d %-12s unit %.3e  bar %.3e  error %.3e" % (src_size, dst_size, C, name, unit, bar, err))
        assert err <= bar
    tatt_amd.sync_check()


@pytest.mark.parametrize("case", ["B1", "B5", "beyond_capacity"])
def test_two_bilstm_layers_at_the_recogniser_size(dev, case):
    """I = 512, H = 256, T = 25, two stacked layers as ASTER.encode runs them, against float64 nn.LSTM; the tolerances of
    test_lstm_chain_bitwise_and_fp64.  The third batch is the first the one-launch chain declines: the per-step kernels run"""
    T, I, Hd = 25, 512, 256
    groups = min(256, infer.lstm_chain_capacity(dev)) // 32             # row blocks of 16 images the chain launch holds
    assert groups >= 1
    B = {"B1": 1, "B5": 5, "beyond_capacity": 16 * groups + 1}[case]
    gen = torch.Generator().manual_seed(B)
    rnn = torch.nn.LSTM(I, Hd, bidirectional=True, num_layers=2)
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.06)
    x = torch.randn(T, B, I, generator=gen)
    rg = torch.nn.LSTM(I, Hd, bidirectional=True, num_layers=2).to(dev)
    rg.load_state_dict(rnn.state_dict())
    with torch.no_grad():
        ref = rnn.double()(x.double())[0]
        xd = x.to(dev)
        gi = infer.lstm_input_projection(xd, rg)
        out, sync = torch.empty(T, B, 2 * Hd, device=dev), torch.zeros(1024, dtype=torch.int32, device=dev)
        rc = LIB.tatt_lstm_fwd_chain(ops.P(gi), ops.P(rg.weight_hh_l0), ops.P(rg.weight_hh_l0_reverse), ops.P(rg.bias_hh_l0),
                                     ops.P(rg.bias_hh_l0_reverse), ops.P(out), ops.P(sync), T, B, Hd, ops.stream())
        assert rc == (1 if case == "beyond_capacity" else 0)           # the chain takes what it holds and declines the rest
        run = lambda chain: infer.bilstm_eval(infer.bilstm_eval(xd, rg, chain=chain), aster._Layer1View(rg), chain=chain)
        a, b = run(True), run(False)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (T, B, 2 * Hd)
    assert torch.equal(a, b), max_err(a, b)
    err = max_err(a, ref)
    print("two BiLSTM layers I=512 T=25 B=%d (%s): error %.3e against float64" % (B, "per-step kernels" if rc else "one launch per layer", err))
    assert err < 1e-5, err
    tatt_amd.sync_check()
