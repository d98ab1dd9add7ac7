"""The MORAN recogniser on the GPU: the rectifier's one-launch tail (tatt_morn_rectify) alone, the stages (`offsets`, `rectify`, `encode`)
under both arithmetic settings, and the whole recogniser (`read`, `forward`, `io.evaluate`) against what the reference recorded
(tests/golden/moran_e2e.npz, tools/gen_golden_moran.py) and against the float64 specification of tests/moran_ref.py.
Every convolution route as a single layer, and the stages at batch 1, 2, 5 and 48 with the contraction split on and off, are in
tests/test_moran_routes_gpu.py.

Error bars: 4 x the recorded distance of the reference's own fp32 result from its float64 run at that stage + 1e-7 x the largest |value|;
for the sampler alone, 4 x the recorded distance of the reference's fp32 sampler from float64 sampling at the same recorded offsets."""
import os

import numpy as np
import pytest
import torch

import tatt_amd
from tatt_amd import io, moran, ops
from tatt_amd._lib import LIB

import moran_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
SIZE = (32, 100)
_CACHE = {}


@pytest.fixture(scope="module")
def e2e():
    return np.load(os.path.join(GOLD, "moran_e2e.npz"))


@pytest.fixture(scope="module")
def model():
    return R.e2e_model(tatt_amd.MORAN).to(DEV).eval()


@pytest.fixture
def arithmetic(request):
    before = tatt_amd.get_arithmetic()
    tatt_amd.set_arithmetic(request.param)
    yield request.param
    tatt_amd.set_arithmetic(before if before != "mixed" else "split_bf16")


def _bar(e2e, err_key, maxabs):
    return 4.0 * float(e2e[err_key]) + 1e-7 * float(maxabs)


def _dist(got, want):
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - np.asarray(want, dtype=np.float64)).max())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _slice_of_channels_last(img, c=2):
    """the image as channel c of a channels-last 4-channel tensor: element strides (H * W * 4, 1, W * 4, 4)"""
    B, _, H, W = img.shape
    x4 = torch.rand(B, 4, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    x4[:, c] = img[:, 0]
    x = x4[:, c:c + 1]
    assert x.stride(3) == 4 and not x.is_contiguous()
    return x


# ---- tatt_morn_rectify alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_rectify_kernel_at_the_recorded_offsets(B, e2e):
    img = _dev(e2e["images"][:B])
    x = _slice_of_channels_last(img)
    o1, o2 = _dev(e2e["offsets"][:B]), _dev(e2e["offsets2"][:B])
    want_grid, want_rect = e2e["offsets_grid"][:B], e2e["rect"][:B]
    bar_g = _bar(e2e, "err_grid_at_offsets", np.abs(e2e["offsets_grid"]).max())
    bar_r = _bar(e2e, "err_rect_at_offsets", np.abs(e2e["rect"]).max())
    # the first pass: offsets_grid = g(o1), against float64 at the same recorded o1
    rect1, acc = moran.morn_rectify(o1, x, SIZE)
    assert tuple(rect1.shape) == (B, 32, 100, 1) and tuple(acc.shape) == (B, 32, 100)
    d_first = _dist(acc, R.offsets_increment(e2e["offsets"][:B], SIZE))
    d_rect1 = _dist(rect1[..., 0], R.rectify_at(e2e["images"][:B], acc.cpu().numpy())[:, 0])
    # the accumulating pass, in place
    rect, acc2 = moran.morn_rectify(o2, x, SIZE, acc)
    assert acc2.data_ptr() == acc.data_ptr()
    d_grid = _dist(acc2, want_grid)
    d_rect = _dist(rect[..., 0], R.rectify_at(e2e["images"][:B], acc2.cpu().numpy())[:, 0])
    # the sampler alone at the RECORDED offsets: a zero map adds nothing to them
    acc3 = _dev(want_grid)
    rect3, _ = moran.morn_rectify(torch.zeros_like(o1), x, SIZE, acc3)
    assert np.array_equal(acc3.cpu().numpy(), want_grid)
    d_rec = _dist(rect3[..., 0], want_rect[:, 0])
    print("rectify kernel B=%d: first offsets_grid %.3e, accumulated %.3e (bar %.3e); image at its own offsets %.3e / %.3e, at the recorded "
          "ones vs the recording %.3e (bar %.3e)" % (B, d_first, d_grid, bar_g, d_rect1, d_rect, d_rec, bar_r))
    assert d_first <= bar_g and d_grid <= bar_g
    assert d_rect1 <= bar_r and d_rect <= bar_r and d_rec <= bar_r


def test_rectify_kernel_zeros_padding():
    """A synthetic map with values up to +-1.5 pushes samples above and below the image: the zeros-padding path, against moran_ref.
    Bars (derived): a sampling coordinate takes at most 4 roundings of 2^-24 relative.  In the image it reaches 64 pixels (1.5e-5 pixel), an
    image in [0, 1] changes by at most 1 per pixel, and the four weights add 4 x 2^-24: 2e-5.  In the pooled map it reaches 12 pixels
    (2.9e-6 pixel) and the map, within +-1.5, changes by at most 3 per pixel: 1e-5 per pass with the weights' share, 2e-5 for the sum of
    two.  Three channels, plain NCHW strides."""
    g = torch.Generator().manual_seed(21)
    B = 2
    o = (torch.rand(B, 4, 12, generator=g) * 3.0 - 1.5)
    o2 = (torch.rand(B, 4, 12, generator=g) * 3.0 - 1.5)
    img = torch.cat([R.images(B, seed=30 + c) for c in range(3)], 1)
    x = img.to(DEV)
    rect1, acc = moran.morn_rectify(o.to(DEV), x, SIZE)
    want1 = R.offsets_increment(o.numpy(), SIZE)
    assert _dist(acc, want1) <= 1e-5
    rect, acc = moran.morn_rectify(o2.to(DEV), x, SIZE, acc)
    og = acc.cpu().numpy()
    assert _dist(acc, want1 + R.offsets_increment(o2.numpy(), SIZE)) <= 2e-5
    want = R.rectify_at(img.numpy(), og)
    assert og.max() > 1.2 and og.min() < -1.2
    sy = np.linspace(-1, 1, 32)[None, :, None] + og
    out_rows = (sy > 1.1) | (sy < -1.1)
    assert out_rows.mean() > 0.1 and (~out_rows).mean() > 0.1                   # samples beyond both edges, and samples inside
    got = rect.permute(0, 3, 1, 2).cpu().numpy()
    assert np.all(got[np.broadcast_to(out_rows[:, None], got.shape)] == 0.0)    # beyond the edge (and its half pixel): exactly zero
    d = float(np.abs(got - want).max())
    print("rectify kernel, zeros padding: offsets_grid spans %.2f .. %.2f, %.0f%% of the samples outside, image error %.3e (bar 2e-5)"
          % (og.min(), og.max(), 100 * out_rows.mean(), d))
    assert d <= 2e-5


def test_rectify_kernel_other_extents(e2e):
    """targetW = 50: the offsets map is 4 x 6 and the grid 32 x 50"""
    g = torch.Generator().manual_seed(22)
    B, size = 3, (32, 50)
    o = torch.rand(B, 4, 6, generator=g) * 0.8 - 0.4
    img = R.images(B, seed=40, W=50)
    rect, acc = moran.morn_rectify(o.to(DEV), img.to(DEV), size)
    assert tuple(rect.shape) == (B, 32, 50, 1)
    d_g = _dist(acc, R.offsets_increment(o.numpy(), size))
    d_r = _dist(rect[..., 0], R.rectify_at(img.numpy(), acc.cpu().numpy())[:, 0])
    bar_g = _bar(e2e, "err_grid_at_offsets", np.abs(e2e["offsets_grid"]).max())
    bar_r = _bar(e2e, "err_rect_at_offsets", np.abs(e2e["rect"]).max())
    print("rectify kernel 32 x 50: offsets_grid %.3e (bar %.3e), image %.3e (bar %.3e)" % (d_g, bar_g, d_r, bar_r))
    assert d_g <= bar_g and d_r <= bar_r


def test_rectify_kernel_refusals():
    z = torch.zeros(8, device=DEV)
    p = ops.P(z)
    s = (3200, 3200, 100, 1)
    call = lambda h, w, C, Ho=32, Wo=100: LIB.tatt_morn_rectify(p, h, w, p, 1, p, *s, p, 1, C, 32, 100, Ho, Wo, ops.stream())
    # (the entry refuses before it launches)
    assert call(1, 12, 1) == 1 and call(4, 1, 1) == 1 and call(4, 12, 5) == 1 and call(4, 12, 1, 1, 100) == 1 and call(65, 64, 1) == 1


# ---- the stages ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", ["split_bf16", "fp32"], indirect=True)
def test_stages_against_the_recording(arithmetic, model, e2e):
    x = _dev(e2e["images"])
    with torch.no_grad():
        o = model.offsets(x)
        rect, og = model.rectify(x, want_offsets=True)
        feats = model.encode(_dev(e2e["rect"]).permute(0, 2, 3, 1))
    res = [("offsets", _dist(o, e2e["offsets"])), ("offsets_grid", _dist(og, e2e["offsets_grid"])),
           ("rect", _dist(rect.permute(0, 3, 1, 2), e2e["rect"])), ("feats", _dist(feats, e2e["feats"]))]
    assert tuple(o.shape) == (R.E2E_B, 4, 12) and tuple(feats.shape) == (R.E2E_B, 25, 256)
    bars = {k: _bar(e2e, "err_" + k, np.abs(e2e[k]).max()) for k, _ in res}
    for k, d in res:
        print("%s stage %-12s: distance from the recording %.3e, bar %.3e" % (arithmetic, k, d, bars[k]))
    for k, d in res:
        assert d <= bars[k], (k, d, bars[k])


def _narrow():
    if "narrow" not in _CACHE:
        m = R.e2e_model(tatt_amd.MORAN, targetW=50)
        img = R.images(3, seed=41, W=50)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        spec = R.rectifier(sd, img.numpy())
        spec["feats"] = R.feats(sd, spec["rect"])
        _CACHE["narrow"] = (m.to(DEV).eval(), img, spec)
    return _CACHE["narrow"]


@pytest.mark.parametrize("arithmetic", ["split_bf16", "fp32"], indirect=True)
def test_stages_at_an_odd_width(arithmetic, e2e):
    """MORAN(1, 37, 256, 32, 50): the offsets map is 4 x 6 and the strided 3 x 3 convolutions meet an odd-width map (25 -> 13, T = 13);
    against the float64 specification, within the fixture's bars"""
    m, img, spec = _narrow()
    x = img.to(DEV)
    with torch.no_grad():
        o = m.offsets(x)
        rect, og = m.rectify(x, want_offsets=True)
        feats = m.encode(_dev(spec["rect"].astype(np.float32)).permute(0, 2, 3, 1))
    assert tuple(o.shape) == (3, 4, 6) and tuple(feats.shape) == (3, 13, 256)
    res = [("offsets", _dist(o, spec["offsets"])), ("offsets_grid", _dist(og, spec["offsets_grid"])),
           ("rect", _dist(rect.permute(0, 3, 1, 2), spec["rect"])), ("feats", _dist(feats, spec["feats"]))]
    bars = {k: _bar(e2e, "err_" + k, np.abs(e2e[k]).max()) for k, _ in res}
    for k, d in res:
        print("%s W=50 stage %-12s: distance from float64 %.3e, bar %.3e" % (arithmetic, k, d, bars[k]))
    for k, d in res:
        assert d <= bars[k], (k, d, bars[k])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_read_gives_the_recorded_strings(model, e2e):
    x = _dev(e2e["images"])
    before = dict(moran.LAUNCHES)
    ids, logits = model.read(x)
    assert moran.LAUNCHES["one_launch"] == before["one_launch"] + 1 and moran.LAUNCHES["eager"] == before["eager"]
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (R.E2E_B, 20) and tuple(logits.shape) == (R.E2E_B, 20, 37)
    assert moran.get_string_moran(ids) == [str(s) for s in e2e["strings"]]
    assert np.array_equal(ids.cpu().numpy(), e2e["ids_l2r"])                     # (every row's margin is above the bound: test_moran.py)
    rids, _ = model.read(x, reverse=True)
    assert np.array_equal(rids.cpu().numpy(), e2e["ids_r2l"])
    ids5, _ = model.read(x[:2], steps=5)
    assert np.array_equal(ids5.cpu().numpy(), e2e["ids_l2r"][:2, :5])
    with pytest.raises(ValueError, match="reads"):
        model.read(x[:, :, :, :64])


def test_forward_rows_in_the_reference_layout(model, e2e):
    x = _dev(e2e["images"])
    full = [20] * R.E2E_B
    l2r, r2l = model(x, torch.tensor(full, dtype=torch.int32), None, None, test=True)
    for name, got in (("l2r", l2r), ("r2l", r2l)):
        assert tuple(got.shape) == (R.E2E_B * 20, 37)
        d, bar = _dist(got, e2e["logits_" + name]), _bar(e2e, "err_logits_" + name, e2e["max_logits_" + name])
        print("forward rows %s: distance from the recording %.3e, bar %.3e" % (name, d, bar))
        assert d <= bar
    lens = [20, 5, 20, 1, 13, 20]
    want = {n: R.rows(e2e["logits_" + n].reshape(R.E2E_B, 20, 37), lens) for n in ("l2r", "r2l")}
    l2r, r2l = model(x, torch.tensor(lens, dtype=torch.int32).to(DEV), None, None, test=True)      # (a device tensor is copied)
    assert tuple(l2r.shape) == (sum(lens), 37)
    assert _dist(l2r, want["l2r"]) <= _bar(e2e, "err_logits_l2r", e2e["max_logits_l2r"])
    assert _dist(r2l, want["r2l"]) <= _bar(e2e, "err_logits_r2l", e2e["max_logits_r2l"])
    preds, demo = model(x, lens, None, None, test=True, debug=True)
    assert demo is None and torch.equal(preds[0], l2r)


def test_evaluate_with_moran(model, monkeypatch):
    torch.manual_seed(5)
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    batches = [(torch.rand(3, 4, 16, 64, generator=g).to(DEV), torch.rand(3, 4, 32, 128, generator=g).to(DEV)) for _ in range(2)]
    # the host restatement of the loop, from the same calls: the labels are made from what it reads (some right, some wrong)
    strings = {"sr": [], "lr": [], "hr": []}
    with torch.no_grad():
        for lr, hr in batches:
            sr = gen(lr)
            sr = sr[0] if isinstance(sr, tuple) else sr
            for name, im in (("sr", sr), ("lr", lr), ("hr", hr)):
                t, length, text, _ = moran.parse_moran_data(im[:, :3])
                assert tuple(t.shape) == (3, 1, 32, 100) and length.tolist() == [20] * 3 and text.numel() == 60
                strings[name] += moran.get_string_moran(model.read(t, 20)[0])
    labels = [strings["sr"][0], "zz9", strings["lr"][2], strings["hr"][3], strings["sr"][4], "nothing"]
    full = [(lr, hr, None, labels[3 * i:3 * i + 3]) for i, (lr, hr) in enumerate(batches)]
    want = {k: round(sum(io.str_filt(p, "lower") == io.str_filt(t, "lower") for p, t in zip(strings[k], labels)) / 6, 4) for k in strings}
    torch.cuda.synchronize()
    count = {"n": 0}
    for meth in ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__"):
        orig = getattr(torch.Tensor, meth)

        def wrapped(self, *a, _orig=orig, **k):
            if self.is_cuda:
                count["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, wrapped)
    res = io.evaluate(gen, full, recognizer=model, full_metrics=True)
    monkeypatch.undo()
    assert count["n"] == 1, "io.evaluate read the device %d times" % count["n"]
    assert res["n_images"] == 6 and res["n_batches"] == 2
    assert (res["accuracy"], res["accuracy_lr"], res["accuracy_hr"]) == (want["sr"], want["lr"], want["hr"])
    assert res["accuracy"] >= round(2 / 6, 4)
    for k in ("psnr", "ssim", "psnr_lr", "ssim_lr", "ned", "ned_lr", "ned_hr", "ned_skipped"):
        assert k in res and np.isfinite(res[k])
    assert set(res) == {"psnr", "ssim", "n_batches", "psnr_lr", "ssim_lr", "accuracy", "accuracy_lr", "accuracy_hr", "n_images", "ned",
                        "ned_lr", "ned_hr", "ned_skipped"}
    assert not model.training
    tatt_amd.sync_check()
