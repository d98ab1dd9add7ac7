"""The MORAN recogniser's rectifier network and encoder against float64 at every route the evaluation loop can take, beyond the recorded
fixture (batch 6) and the odd-width run (batch 3) of tests/test_moran_gpu.py:

  1. every distinct convolution geometry of MORN.cnn and of ASRN's ResNet -- walked from the modules as `MORAN.offsets` and `MORAN.encode`
     run them, not listed -- as ONE layer through `ops.conv2d_forward`, filter and bias from `infer.bn_fold`, the input the view the model
     hands over (a dense NHWC map; `o[:, ::sh, ::sw, :]` of one for the 3 x 3 conv2 of a group's first block; both layouts of the one-channel
     image for block0; the pooled channel slice for MORN.cnn.1), on both sides of the batch size at which `ops.conv_split` stops splitting
     the contraction.  A strided 3 x 3 runs dense, and its result read at [::sh, ::sw] is compared with float64 F.conv2d at that stride;
  2. the rectifier, the encoder and the reader at batch 1, 2, 5 and 48, as shipped and with CONV_SPLIT_TILES = 0, under both arithmetic
     settings.  Batch 48 (the evaluation loop's) is the mixed configuration: the geometries whose boundary is 40 / 41 run unsplit, the rest
     of the deep ones split.

Oracles: tests/moran_ref.py (pinned on the CPU by tests/test_moran.py against what the reference recorded) and torch's float64 operators.
Error bars of 2.: 4 x the distance of the same oracle run in float32 on the CPU from its float64 run on the same inputs, measured inside
the test, + 1e-7 x the largest |value|.  The single layers use `check_close` at the tolerances of test_conv2d_fn (rtol 2e-4, atol 2e-5,
weights scaled by 1 / sqrt(Cin k k)).

Measured on the MI355X (unit = float32 CPU run of the specification against its float64 run, on that machine's host; bar = 4 x unit +
1e-7 x max; error = GPU against float64; both arithmetic settings gave the same figures: no kernel of this path depends on the setting):
  batch  stage                 unit       bar        error as shipped   error with CONV_SPLIT_TILES = 0
  1      offsets               4.513e-07  1.870e-06  2.578e-07          3.770e-07
  1      offsets_grid          8.067e-07  3.358e-06  7.596e-07          8.490e-07
  1      rect                  8.586e-06  3.444e-05  6.919e-06          5.369e-06
  1      encode(oracle rect)   1.434e-06  5.754e-06  1.355e-06          2.214e-06
  1      feats                 2.009e-06  8.052e-06  1.826e-06          2.294e-06
  1      logits L2R            1.786e-06  9.081e-06  6.923e-06          6.447e-06
  1      logits R2L            2.080e-06  1.001e-05  6.038e-06          6.395e-06
  2      offsets               2.878e-07  1.218e-06  4.680e-07          5.467e-07
  2      offsets_grid          7.427e-07  3.104e-06  1.006e-06          7.317e-07
  2      rect                  3.498e-06  1.409e-05  5.793e-06          6.999e-06
  2      encode(oracle rect)   1.515e-06  6.079e-06  4.771e-06          3.408e-06
  2      feats                 2.024e-06  8.113e-06  3.463e-06          3.873e-06
  2      logits L2R            3.137e-06  1.449e-05  8.336e-06          8.120e-06
  2      logits R2L            3.964e-06  1.755e-05  5.526e-06          7.006e-06
  5      offsets               4.714e-07  1.952e-06  4.886e-07          4.584e-07
  5      offsets_grid          6.743e-07  2.832e-06  8.653e-07          1.078e-06
  5      rect                  4.403e-06  1.771e-05  6.473e-06          8.818e-06
  5      encode(oracle rect)   2.590e-06  1.038e-05  3.464e-06          3.393e-06
  5      feats                 1.833e-06  7.348e-06  3.165e-06          4.875e-06
  5      logits L2R            2.444e-06  1.171e-05  6.211e-06          7.393e-06
  5      logits R2L            2.775e-06  1.280e-05  6.899e-06          7.017e-06
  48     offsets               4.746e-07  1.967e-06  7.675e-07          8.278e-07
  48     offsets_grid          1.019e-06  4.212e-06  9.498e-07          1.054e-06
  48     rect                  7.636e-06  3.065e-05  1.072e-05          1.237e-05
  48     encode(oracle rect)   2.984e-06  1.195e-05  5.876e-06          5.042e-06
  48     feats                 3.933e-06  1.575e-05  7.132e-06          6.366e-06
  48     logits L2R            5.597e-06  2.433e-05  1.044e-05          1.214e-05
  48     logits R2L            8.003e-06  3.371e-05  1.383e-05          1.499e-05
  ids: 0 of 48 rows below the margin bound in both directions (smallest float64 margins 0.17 and 0.067, needs 2.0e-3 and 2.2e-3);
  offsets_grid spans -1.36 .. 0.47, mean |rect - image| 0.35
What this file found: with CONV_SPLIT_TILES = 0 (the configuration of batch >= 82) the im2col kernel summed a contraction of up to 4608
products in ONE fp32 chain, and `feats` missed its bar at batch 2 (9.405e-06 against 8.113e-06) and batch 5 (9.570e-06 against 7.348e-06,
both logits with it: 1.291e-05 / 1.171e-05 and 1.493e-05 / 1.280e-05) while every single layer passed.  An unsplit contraction of 64
chunks and more now sums in blocks of 32 chunks (gemm_fast_kernel's BLOCKED variant); the table is measured with it.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tatt_amd
from tatt_amd import infer, moran, ops
from tatt_amd.ops import ACT_NONE, ACT_RELU

import moran_ref as R
from tests.util import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS32 = float(torch.finfo(torch.float32).eps)
BATCH_LIMIT = 256                  # MORN's maxBatch; a split boundary above it is reached with CONV_SPLIT_TILES = 0 at batch 3 instead
SIZE = (32, 100)


# ---- 1. single layers ------------------------------------------------------------------------------------------------------------------
def _geometries():
    """{(H, W, Cin, Cout, k, (vh, vw), (sh, sw), act, layout): first layer of that geometry}.  H x W is the map the convolution runs on;
    (vh, vw) != (1, 1): its input is the [::vh, ::vw] view of a dense map; (sh, sw) != (1, 1): the layer has that stride, runs dense and its
    result is read at [::sh, ::sw]; layout: 'dense', 'nchw' (the NHWC view of an NCHW tensor) or 'slice' (pooled from a channel slice)"""
    found = {}

    def add(where, H, W, conv, view, sub, act, layout="dense"):
        k = conv.kernel_size[0]
        assert conv.kernel_size == (k, k) and conv.padding == (k // 2, k // 2) and tuple(conv.stride) == tuple(sub), where
        assert conv.bias is not None, where
        found.setdefault((H, W, conv.in_channels, conv.out_channels, k, tuple(view), tuple(sub), act, layout), where)

    with torch.device("meta"):                                         # (shapes only: no parameters are drawn)
        m = moran.MORAN(R.KW["nc"], R.KW["nclass"], R.KW["nh"], R.KW["targetH"], R.KW["targetW"], BidirDecoder=True)
    # MORAN.offsets: a 2 x 2 pool, then the convolutions, a pool after two of them, ReLU after all but the last
    H, W = SIZE[0] // 2, SIZE[1] // 2
    for i in moran.MORN_CONVS:
        act = ACT_RELU if i != moran.MORN_CONVS[-1] else ACT_NONE
        add("MORN.cnn.%d" % i, H, W, m.MORN.cnn[i], (1, 1), (1, 1), act)
        if i == moran.MORN_CONVS[0]:
            add("MORN.cnn.%d" % i, H, W, m.MORN.cnn[i], (1, 1), (1, 1), act, "slice")
        if i in moran.MORN_POOL_AFTER:
            H, W = H // 2, W // 2
    assert (H, W) == (4, 12)
    # MORAN.encode
    cnn = m.ASRN.cnn
    H, W = SIZE
    add("block0", H, W, cnn.block0[0], (1, 1), (1, 1), ACT_NONE)
    add("block0", H, W, cnn.block0[0], (1, 1), (1, 1), ACT_NONE, "nchw")
    for li in range(1, 6):
        for bi, blk in enumerate(getattr(cnn, "block%d" % li)):
            name = "block%d.%d." % (li, bi)
            sh, sw = blk.stride
            if blk.downsample is not None:
                add(name + "conv1", H, W, blk.conv1[0], (1, 1), (sh, sw), ACT_NONE)
                add(name + "downsample", H, W, blk.downsample[0], (1, 1), (sh, sw), ACT_NONE)
                H, W = len(range(0, H, sh)), len(range(0, W, sw))      # the size of o[:, ::sh, ::sw, :]
                add(name + "conv2", H, W, blk.conv2[0], (sh, sw), (1, 1), ACT_NONE)
            else:
                assert (sh, sw) == (1, 1)
                add(name + "conv1", H, W, blk.conv1[0], (1, 1), (1, 1), ACT_NONE)
                add(name + "conv2", H, W, blk.conv2[0], (1, 1), (1, 1), ACT_NONE)
    assert (H, W) == (1, 25)
    return found


GEOMS = _geometries()


def _gid(g):
    H, W, Cin, Cout, k, (vh, vw), (sh, sw), act, layout = g
    return "%s-%dx%d-%dto%d-k%d-view%dx%d-sub%dx%d-%s-%s" % (GEOMS[g], H, W, Cin, Cout, k, vh, vw, sh, sw,
                                                             "relu" if act == ACT_RELU else "none", layout)


def _key(g):
    return "%s:%dx%d:%d->%d:k%d" % (GEOMS[g], g[0], g[1], g[2], g[3], g[4])


def _splits(g, B):
    H, W, Cin, Cout, k = g[:5]
    return ops.conv_split(torch.empty(B, H, W, Cin, device="meta"), Cout, k, k)


def _boundary(g):
    """None: the geometry never splits; B: the smallest batch that does not split (B - 1 does); BATCH_LIMIT + 1: it splits up to the limit"""
    if _splits(g, 1) == 1:
        assert all(_splits(g, B) == 1 for B in (2, 3, 5, 48, 64, BATCH_LIMIT))
        return None
    for B in range(2, BATCH_LIMIT + 1):
        if _splits(g, B) == 1:
            return B
    return BATCH_LIMIT + 1


def _deep(g):
    """a contraction of 32 chunks of 16 and more: what `conv_split` splits while the output tiles are few"""
    return -(-g[2] * g[4] * g[4] // 16) >= 32


def _ragged_batch(H, W):
    """the smallest batch from 4 on with more than one row tile of 64 pixels and a partial last one (None: H * W is a multiple of 64)"""
    for B in range(4, 70):
        if B * H * W > 64 and (B * H * W) % 64:
            return B
    return None


def test_the_walk_finds_the_split_boundaries_of_the_layer_table():
    """the boundaries `conv_split` gives today, recomputed: if a threshold moves, this names the layer"""
    got = {_key(g): _boundary(g) for g in GEOMS if _boundary(g)}
    print(got)
    over = BATCH_LIMIT + 1
    want = {"MORN.cnn.5:8x25:64->128:k3": 41, "MORN.cnn.9:4x12:128->64:k3": over, "MORN.cnn.12:4x12:64->16:k3": over,
            "block2.0.conv2:8x25:64->64:k3": 82, "block2.1.conv2:8x25:64->64:k3": 82,
            "block3.0.conv1:8x25:64->128:k3": 41, "block3.0.conv2:4x25:128->128:k3": 82, "block3.1.conv2:4x25:128->128:k3": 82,
            "block4.0.conv1:4x25:128->256:k3": 41, "block4.0.conv2:2x25:256->256:k3": 81, "block4.1.conv2:2x25:256->256:k3": 81,
            "block5.0.conv1:2x25:256->512:k3": 40, "block5.0.conv2:1x25:512->512:k3": 80, "block5.1.conv1:1x25:512->512:k1": 80,
            "block5.1.conv2:1x25:512->512:k3": 80}
    assert got == want
    assert all(_deep(g) == (_boundary(g) is not None) for g in GEOMS)
    assert sum(1 for g in GEOMS if g[3] == 1) >= 1
    assert sum(1 for g in GEOMS if g[3] == 16 and _boundary(g)) >= 1
    assert sum(1 for g in GEOMS if g[2] == 1) >= 2
    assert sum(1 for g in GEOMS if g[3] == 32) >= 1
    assert sum(1 for g in GEOMS if g[4] == 3 and g[5] != (1, 1)) >= 4
    assert {g[8] for g in GEOMS} == {"dense", "nchw", "slice"}


def _slice_of_channels_last(img, gen, c=2):
    """the one-channel image as channel c of a channels-last 4-channel tensor (element stride 4), the other channels noise"""
    B, _, H, W = img.shape
    x4 = torch.rand(B, 4, H, W, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
    x4[:, c] = img[:, 0]
    x = x4[:, c:c + 1]
    assert x.stride(3) == 4 and not x.is_contiguous()
    return x


@pytest.mark.parametrize("g", list(GEOMS), ids=_gid)
def test_conv_geometry_against_float64(dev, g, monkeypatch):
    H, W, Cin, Cout, k, (vh, vw), (sh, sw), act, layout = g
    gen = torch.Generator().manual_seed(100 + list(GEOMS).index(g))
    w = torch.randn(Cout, Cin, k, k, generator=gen) / math.sqrt(Cin * k * k)
    cb = torch.randn(Cout, generator=gen)                               # (every convolution of MORAN has a bias)
    bn = torch.nn.BatchNorm2d(Cout)
    with torch.no_grad():
        bn.running_mean.copy_(0.3 * torch.randn(Cout, generator=gen))
        bn.running_var.copy_(0.5 + torch.rand(Cout, generator=gen))
        bn.weight.copy_(0.5 + torch.rand(Cout, generator=gen))
        bn.bias.copy_(0.3 * torch.randn(Cout, generator=gen))
    bn_dev = torch.nn.BatchNorm2d(Cout).to(dev).eval()
    bn_dev.load_state_dict(bn.state_dict())
    bn.requires_grad_(False), bn_dev.requires_grad_(False)
    wf, bf = infer.bn_fold(w.to(dev), cb.to(dev), bn_dev)
    # the fold against torch fp32 on the device (the host's fp32 square root need not be correctly rounded): w s bitwise or to 1 ulp,
    # (b - mean) s + beta to 1 ulp of its larger term (the kernel may contract it)
    s = bn_dev.weight / torch.sqrt(bn_dev.running_var + bn_dev.eps)
    w_want = w.to(dev) * s.view(-1, 1, 1, 1)
    assert bool(((wf - w_want).abs() <= EPS32 * w_want.abs()).all())
    t = cb.to(dev) - bn_dev.running_mean
    b_want = t.double() * s.double() + bn_dev.bias.double()
    assert bool(((bf.double() - b_want).abs() <= EPS32 * ((t * s).abs() + bn_dev.bias.abs()).double()).all())

    def bn64(v):
        shape = (1, -1, 1, 1)
        return ((v - bn.running_mean.double().view(shape)) / torch.sqrt(bn.running_var.double().view(shape) + bn.eps)
                * bn.weight.double().view(shape) + bn.bias.double().view(shape))

    bnd = _boundary(g)
    if bnd is None:
        rb = _ragged_batch(H, W)
        plan = [(1, False), (3, False), (rb if rb is not None else 5, False)]
    elif bnd > BATCH_LIMIT:
        plan = [(1, False), (3, False), (3, True)]
    else:
        plan = [(1, False), (3, False), (bnd - 1, False), (bnd, False)]
    report, off_side, routes = [], [], set()
    for B, patched in plan:
        if patched:
            monkeypatch.setattr(ops, "CONV_SPLIT_TILES", 0)
        if layout == "slice":
            # what MORAN.offsets does to a strided image before its first convolution; the reference pools the same image
            img = torch.rand(B, Cin, 2 * H, 2 * W, generator=gen)
            xin = ops.maxpool_fwd(ops.to_contiguous(_slice_of_channels_last(img.to(dev), gen).permute(0, 2, 3, 1)), 2, 2)
            x = F.max_pool2d(img.double(), 2, 2)
        else:
            x = torch.randn(B, Cin, H * vh, W * vw, generator=gen)     # the dense map the layer's input is a view of
            xd = x.to(dev)
            if layout == "nchw":
                xin = xd.permute(0, 2, 3, 1)
            else:
                dense = xd.permute(0, 2, 3, 1).contiguous()
                # the pixels the view skips hold values too: a wrong stride picks them up
                xin = dense[:, ::vh, ::vw, :] if (vh, vw) != (1, 1) else dense
                assert xin.stride()[:3] == (dense.stride(0), vh * dense.stride(1), vw * dense.stride(2))
            x = x.double()[:, :, ::vh, ::vw]
        assert tuple(xin.shape) == (B, H, W, Cin)
        splits = ops.conv_split(xin, Cout, k, k)
        report.append("B=%d%s: %d" % (B, " (CONV_SPLIT_TILES=0)" if patched else "", splits))
        want_split = not (bnd is None or patched) and (bnd > BATCH_LIMIT or B < bnd)
        if (splits > 1) != want_split:
            off_side.append((B, patched, splits))
        # (what try_conv_fast takes; the rest runs launch_gemm<3, 16>)
        routes.add(Cout % 64 == 0 and Cin % 16 == 0 and xin.stride(3) == 1 and all(v % 4 == 0 for v in xin.stride()[:3]))
        y = ops.conv2d_forward(xin, wf, bf, act)
        assert tuple(y.shape) == (B, H, W, Cout) and y.is_contiguous()
        assert act in (ACT_RELU, ACT_NONE)
        ref = bn64(F.conv2d(x, w.double(), cb.double(), padding=k // 2))
        ref = torch.relu(ref) if act == ACT_RELU else ref
        tag = "%s B=%d splits=%d" % (_gid(g), B, splits)
        check_close(tag, y, ref.permute(0, 2, 3, 1), rtol=2e-4, atol=2e-5)
        if (sh, sw) != (1, 1):
            # the layer has a stride: the model reads the dense result at [::sh, ::sw]; float64 at that stride is the reference
            strided = bn64(F.conv2d(x, w.double(), cb.double(), stride=(sh, sw), padding=k // 2))
            yv = y[:, ::sh, ::sw, :]
            assert tuple(yv.shape) == (B, len(range(0, H, sh)), len(range(0, W, sw)), Cout)
            check_close(tag + " read at [::%d, ::%d]" % (sh, sw), yv, strided.permute(0, 2, 3, 1), rtol=2e-4, atol=2e-5)
        if GEOMS[g].endswith("conv2"):                                 # relu(o + residual) follows it
            res = torch.randn(y.shape, generator=gen).to(dev)
            assert torch.equal(moran.add_relu(y, res), torch.relu(y + res))
    assert len(routes) == 1
    print("%s [%s]%s split counts %s" % (_gid(g), "im2col fast route" if routes.pop() else "general route",
                                         "" if bnd is None or bnd > BATCH_LIMIT else " boundary %d | %d" % (bnd - 1, bnd), ", ".join(report)))
    if bnd is None and _ragged_batch(H, W) is None:
        print("    (%d x %d pixels are a multiple of the 64-row tile: no batch leaves a ragged last tile)" % (H, W))
    tatt_amd.sync_check()
    # (asked last, so that a moved threshold still leaves every value compared)
    assert not off_side, "the test no longer straddles the split boundary: (batch, CONV_SPLIT_TILES=0, splits) %s" % off_side


# ---- 2. the rectifier, the encoder and the reader at other batch sizes, split on and off ---------------------------------------------
BATCHES = (1, 2, 5, 48)             # (48: the evaluation loop's default batch)
STEPS = 20
STAGE_LABELS = (("offsets", "offsets"), ("offsets_grid", "offsets_grid"), ("rect", "rect"), ("feats_at_rect", "encode(oracle rect)"),
                ("feats", "feats"), ("logits_l2r", "logits L2R"), ("logits_r2l", "logits R2L"))


@pytest.fixture
def arithmetic(request):
    before = tatt_amd.get_arithmetic()
    tatt_amd.set_arithmetic(request.param)
    yield request.param
    tatt_amd.set_arithmetic(before if before != "mixed" else "split_bf16")


@pytest.fixture(scope="module")
def world():
    """the fixture's recogniser on the device, and the specification's float64 and float32 runs on seeded images, computed once for the
    images of all batch sizes (every stage is per image in eval mode) and left unchanged"""
    m = R.e2e_model(tatt_amd.MORAN)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    img = R.images(sum(BATCHES), seed=43)
    o64, o32 = R.whole(sd, img, STEPS, torch.float64), R.whole(sd, img, STEPS, torch.float32)
    rect_in = torch.from_numpy(o64["rect"]).float()                    # the oracle's own rectified image, as the device receives it
    o64["feats_at_rect"], o32["feats_at_rect"] = R.feats(sd, rect_in.double(), torch.float64), R.feats(sd, rect_in, torch.float32)
    # the fixture exercises the rectifier: the offsets move pixels, some of them beyond the image's edge
    assert np.abs(o64["offsets_grid"]).max() > 0.25 and np.abs(o64["rect"] - img.numpy()).mean() > 0.05
    print("offsets_grid spans %.2f .. %.2f, mean |rect - image| %.2f"
          % (o64["offsets_grid"].min(), o64["offsets_grid"].max(), np.abs(o64["rect"] - img.numpy()).mean()))
    lo, rows = 0, {}
    for B in BATCHES:
        rows[B] = slice(lo, lo + B)
        lo += B
    return {"model": m.to(DEV).eval(), "img": img, "rect_in": rect_in, "o64": o64, "o32": o32, "rows": rows,
            "e2e": np.load(os.path.join(GOLD, "moran_e2e.npz"))}


@pytest.mark.parametrize("arithmetic", ["split_bf16", "fp32"], indirect=True)
@pytest.mark.parametrize("split", ["shipped", "no_split"])
@pytest.mark.parametrize("B", BATCHES)
def test_rectifier_encoder_and_reader_at_batch(world, B, split, arithmetic, monkeypatch):
    deep = [g for g in GEOMS if _deep(g)]
    if split == "no_split":
        monkeypatch.setattr(ops, "CONV_SPLIT_TILES", 0)
        configured = all(_splits(g, B) == 1 for g in GEOMS)
    elif B < 40:
        configured = len(deep) == 15 and all(_splits(g, B) > 1 for g in deep)
    else:
        # the mixed configuration: exactly the geometries whose boundary is reached run unsplit
        unsplit = {_key(g) for g in deep if _splits(g, B) == 1}
        configured = (unsplit == {_key(g) for g in deep if (_boundary(g) or 0) <= B} and 0 < len(unsplit) < len(deep)
                      and unsplit == {"MORN.cnn.5:8x25:64->128:k3", "block3.0.conv1:8x25:64->128:k3", "block4.0.conv1:4x25:128->256:k3",
                                      "block5.0.conv1:2x25:256->512:k3"})
    m, rows, o64, o32 = world["model"], world["rows"][B], world["o64"], world["o32"]
    x = world["img"][rows].to(DEV)
    if B == 5:                                                         # the strided-input path of `offsets` and `morn_rectify`
        x = _slice_of_channels_last(x, torch.Generator().manual_seed(B))
    else:
        assert x.is_contiguous()
    before = dict(moran.LAUNCHES)
    with torch.no_grad():
        got = {"offsets": m.offsets(x)}
        rect, got["offsets_grid"] = m.rectify(x, want_offsets=True)
        got["rect"] = rect.permute(0, 3, 1, 2)
        got["feats_at_rect"] = m.encode(world["rect_in"][rows].to(DEV).permute(0, 2, 3, 1))
        got["feats"] = m.encode(rect)
        ids = {}
        ids["l2r"], got["logits_l2r"] = m.read(x, STEPS)
        ids["r2l"], got["logits_r2l"] = m.read(x, STEPS, reverse=True)
    assert moran.LAUNCHES["one_launch"] == before["one_launch"] + 2 and moran.LAUNCHES["eager"] == before["eager"]
    assert tuple(got["offsets"].shape) == (B, 4, 12) and tuple(got["rect"].shape) == (B, 1) + SIZE
    assert tuple(got["feats"].shape) == (B, 25, 256) and tuple(got["logits_l2r"].shape) == (B, STEPS, 37)
    failed = []
    for name, label in STAGE_LABELS:
        want, w32 = np.asarray(o64[name][rows], dtype=np.float64), np.asarray(o32[name][rows], dtype=np.float64)
        unit = float(np.abs(w32 - want).max())
        bar = 4.0 * unit + 1e-7 * float(np.abs(want).max())
        err = float(np.abs(got[name].detach().cpu().numpy().astype(np.float64) - want).max())
        print("B=%d %-8s %-10s %-20s unit %.3e  bar %.3e  error %.3e" % (B, split, arithmetic, label, unit, bar, err))
        if not err <= bar:
            failed.append((label, err, bar))
    assert not failed, failed
    e2e = world["e2e"]
    for dn in ("l2r", "r2l"):
        _, need = R.margin_bound(e2e["err_logits_" + dn], e2e["max_logits_" + dn])
        margin = o64["margin_" + dn][rows]
        keep = margin > need
        print("B=%d ids %s: %d of %d rows below the margin %.3e (smallest margin %.3e)" % (B, dn, int((~keep).sum()), B, need, margin.min()))
        assert (~keep).sum() * 4 <= len(keep), "more than a quarter of the rows are below the margin bound: %s" % margin
        have = ids[dn].cpu().numpy()
        assert have.dtype == np.int32 and have.shape == (B, STEPS)
        for i in np.nonzero(keep)[0]:
            assert np.array_equal(have[i], o64["ids_" + dn][rows][i]), (dn, i, have[i], o64["ids_" + dn][rows][i])
    tatt_amd.sync_check()
    # (asked last, so that a moved threshold still leaves every value compared)
    assert configured, "the deep convolutions are not split as intended (%s) at batch %d" % (split, B)
