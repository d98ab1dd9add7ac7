"""Device collation on the GPU (tatt_amd.io.DeviceCollator, csrc/collate.hip).  Yardstick: the host path `io.collate_pil_batch` (Pillow +
torch on the CPU), itself pinned to the reference's collate by tests/golden/collate.npz.  Everything after the decode is integer
arithmetic on uint8 pixels, so every comparison is exact (torch.equal): there is no tolerance in this file."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_ref as R

pytestmark = pytest.mark.gpu


def _same(got, want, members=(0, 2, 4, 3)):
    for m in members:
        g, w = got[m], want[m]
        assert g.shape == w.shape and g.dtype == w.dtype and g.device == w.device and g.is_contiguous(), m
        bad = int((g != w).sum())
        assert torch.equal(g, w), "member %d: %d of %d elements differ, max |diff| %g" % (m, bad, g.numel(), float((g - w).abs().max()))
    assert got[1] is None and tuple(got[5]) == tuple(want[5])
    assert torch.equal(got[6], want[6]) and torch.equal(got[7], want[7]) and torch.equal(got[8], want[8])


def test_golden_fixture_of_the_reference_collate(dev):
    from tatt_amd import io
    z = np.load("tests/golden/collate.npz")
    n, alphabet = int(z["n"]), str(z["alphabet"])
    samples = []
    for i in range(n):
        hr, lr = Image.fromarray(z["hr%d" % i], "RGB"), Image.fromarray(z["lr%d" % i], "RGB")
        samples.append((hr, lr, hr, lr, io.str_filt(str(z["labels_in"][i]), "lower")))
    out = io.DeviceCollator(imgH=32, imgW=128, down_sample_scale=2, mask=True, device=dev, alphabet=alphabet)(samples)
    images_HR, pseudo, images_lr, images_HRy, images_lry, label_strs, label_vecs, wmask, wtics = out
    assert pseudo is None and images_HRy is None and images_lry is None
    assert list(label_strs) == [str(v) for v in z["label_strs"]]
    assert images_HR.device.type == "cuda" and label_vecs.device.type == "cuda"
    assert torch.equal(images_HR.cpu(), torch.from_numpy(z["images_HR"])) and torch.equal(images_lr.cpu(), torch.from_numpy(z["images_lr"]))
    assert torch.equal(label_vecs.cpu(), torch.from_numpy(z["label_vecs"]))
    assert torch.equal(wmask, torch.from_numpy(z["weighted_mask"])) and torch.equal(wtics, torch.from_numpy(z["weighted_tics"]))


@pytest.mark.parametrize("imgH,imgW,mask", [(32, 128, True), (32, 128, False), (64, 256, True)],
                         ids=["std-mask", "std-3planes", "large-tile"])
def test_realistic_batch_equals_the_host_path(dev, imgH, imgW, mask):
    from tatt_amd import io
    samples = R.make_batch(2024, B=48)
    want = io.collate_pil_batch(samples, imgH=imgH, imgW=imgW, down_sample_scale=2, mask=mask, device=dev)
    got = io.DeviceCollator(imgH=imgH, imgW=imgW, down_sample_scale=2, mask=mask, device=dev, want_yuv=True)(samples)
    assert tuple(got[0].shape) == (48, 4 if mask else 3, imgH, imgW)
    _same(got, want)
    lean = io.DeviceCollator(imgH=imgH, imgW=imgW, down_sample_scale=2, mask=mask, device=dev, want_yuv=False)(samples)
    assert lean[3] is None and lean[4] is None
    _same(lean, want, members=(0, 2))


def test_route_boundaries_equal_the_host_path(dev):
    """every route of the kernel and the host fallback: a pass skipped (width only, height only, both), up-scaling, one-pixel sides, sources
    at the limits of tatt_collate_limits, one row / column below and one above (above: PIL resizes on the host, the device only converts)"""
    from tatt_amd import io
    lim = io.collate_limits()
    rows, cols, inter = lim["rows"], lim["cols"], lim["inter_bytes"]
    hr_shapes = [(50, 128), (32, 300), (32, 128), (3, 5), (1, 1), (1, 90), (70, 1), (33, 129),
                 (rows, 200), (rows - 1, 200), (rows + 1, 200), (8, cols), (8, cols - 1), (8, cols + 1),
                 (inter // (128 * 3), 500), (inter // (128 * 3) + 1, 127), (inter // (128 * 3) - 1, 129), (rows, cols), (rows + 1, 128)]
    lr_shapes = [(40, 64), (16, 100), (16, 64), (5, 3), (1, 1), (1, 33), (21, 1), (15, 63),
                 (rows, 64), (rows, 65), (rows + 1, 64), (16, cols), (17, cols), (16, cols + 1),
                 (rows, 70), (rows, 63), (rows - 1, 300), (rows, cols), (16, cols + 1)]
    assert len(hr_shapes) == len(lr_shapes)
    # which of them the plan sends through the fallback: exactly the sources beyond a limit
    beyond = lambda h, w, ow: h > rows or w > cols or (w != ow and h * ow * 3 > inter)
    rng = np.random.default_rng(11)
    samples = []
    for i, ((H, W), (h, w)) in enumerate(zip(hr_shapes, lr_shapes)):
        im = lambda hh, ww, k: Image.fromarray(R.make_image(rng, hh, ww, k % 3), "RGB")
        samples.append((im(H, W, i), im(h, w, i + 1), im(h, w, i + 2), im(H, W, i), "w%d" % i))      # (the Y members cross the sizes over)
    col = io.DeviceCollator(imgH=32, imgW=128, down_sample_scale=2, mask=True, device=dev, want_yuv=True)
    (arrays, desc, _, _), _, _ = col.plan(samples)
    B = len(samples)
    for b, ((H, W), (h, w)) in enumerate(zip(hr_shapes, lr_shapes)):
        assert (tuple(desc[b, 1:3]) == (32, 128) and (H, W) != (32, 128)) == beyond(H, W, 128), (H, W)
        assert (tuple(desc[B + b, 1:3]) == (16, 64) and (h, w) != (16, 64)) == beyond(h, w, 64), (h, w)
    assert sum(beyond(H, W, 128) for H, W in hr_shapes) >= 3 and sum(not beyond(H, W, 128) for H, W in hr_shapes) >= 14
    want = io.collate_pil_batch(samples, imgH=32, imgW=128, down_sample_scale=2, mask=True, device=dev)
    _same(col(samples), want)


def test_every_byte_value_converts_exactly(dev):
    from tatt_amd import io
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    a[..., 1] = a[..., 1][::-1]
    im = Image.fromarray(a, "RGB")
    samples = [(im, im, im, im, "x")]
    want = io.collate_pil_batch(samples, imgH=16, imgW=16, down_sample_scale=1, mask=True, device=dev)
    got = io.DeviceCollator(imgH=16, imgW=16, down_sample_scale=1, mask=True, device=dev, want_yuv=True)(samples)
    _same(got, want)
    assert got[0][0, 0].unique().numel() == 256


def test_intermediate_limit_at_the_large_tile_target(dev):
    """imgH = 64, imgW = 256: the bytes of the horizontally resampled rows bind before the row limit.  Sources at that limit (the kernel's
    largest LDS layouts: 128 x 1024 -> 64 x 256), one row above it (the fallback) and around it; the LR members resample to 128 x 32"""
    from tatt_amd import io
    lim = io.collate_limits()
    top = lim["inter_bytes"] // (256 * 3)
    assert top < lim["rows"]
    hr_shapes = [(top, 500), (top + 1, 500), (top, lim["cols"]), (top - 1, lim["cols"]), (top + 1, 256), (lim["rows"], 256), (top + 1, 255)]
    lr_shapes = [(lim["rows"], lim["cols"]), (lim["rows"], 129), (2 * top, 500), (2 * top + 1, 500), (64, 250), (top, 128), (33, 77)]
    rng = np.random.default_rng(17)
    samples = []
    for i, ((H, W), (h, w)) in enumerate(zip(hr_shapes, lr_shapes)):
        im = lambda hh, ww, k: Image.fromarray(R.make_image(rng, hh, ww, k % 3), "RGB")
        samples.append((im(H, W, i), im(h, w, i + 1), im(H, W, i + 2), im(h, w, i), "w%d" % i))
    col = io.DeviceCollator(imgH=64, imgW=256, down_sample_scale=2, mask=True, device=dev, want_yuv=True)
    (_, desc, _, _), _, _ = col.plan(samples)
    B = len(samples)
    fb_hr = [tuple(int(v) for v in desc[b, 1:3]) == (64, 256) for b in range(B)]
    fb_lr = [tuple(int(v) for v in desc[B + b, 1:3]) == (32, 128) for b in range(B)]
    assert fb_hr == [False, True, False, False, False, False, True]
    assert fb_lr == [False, False, False, True, False, False, False]        # (2 * top rows x 128 x 3 bytes is the limit at OW = 128)
    _same(col(samples), io.collate_pil_batch(samples, imgH=64, imgW=256, down_sample_scale=2, mask=True, device=dev))


def test_ring_slots_are_not_overwritten_in_flight(dev):
    """2 * ring + 1 calls on different batches of one size back to back on a side stream, no synchronisation in between (the first call
    allocates the slots, no later one outgrows them: every later reuse of a slot goes through its event alone; that `_slot` waits for it
    is checked without a device in test_collate_device.py)"""
    from tatt_amd import io
    ring = 3
    rng = np.random.default_rng(23)
    shapes = [(int(rng.integers(8, 40)), int(rng.integers(24, 160))) for _ in range(12)]
    batches = []
    for i in range(2 * ring + 1):                                    # the same sizes in every batch, different pixels and labels
        im = lambda hh, ww, k: Image.fromarray(R.make_image(rng, hh, ww, k % 3), "RGB")
        batches.append([(im(2 * h, 2 * w, i + j), im(h, w, j), im(2 * h, 2 * w, j + 1), im(h, w, i), "w%d%d" % (i, j))
                        for j, (h, w) in enumerate(shapes)])
    col = io.DeviceCollator(imgH=32, imgW=128, down_sample_scale=2, mask=True, device=dev, want_yuv=True, ring=ring)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        outs = []
        for b in batches:
            outs.append(col(b))
            assert len(outs) == 1 or col._host[0] is slot0           # never re-allocated
            slot0 = col._host[0]
    side.synchronize()
    for b, got in zip(batches, outs):
        _same(got, io.collate_pil_batch(b, imgH=32, imgW=128, down_sample_scale=2, mask=True, device=dev))


def test_c_layer_refuses_what_it_does_not_take(dev):
    """non-zero return codes, never a fallback inside the C layer: a source beyond the limits, a source that leaves the packed bytes"""
    import ctypes
    from tatt_amd import io, ops
    lim = io.collate_limits()
    packed = torch.zeros(4096, dtype=torch.uint8, device=dev)
    out = torch.zeros(4 * 32 * 128, device=dev)

    def run(row):
        host = torch.tensor(row, dtype=torch.int32)
        d = host.to(dev)
        return ops.LIB.tatt_collate_images(ctypes.c_void_p(packed.data_ptr()), packed.numel(), ctypes.c_void_p(d.data_ptr()),
                                           ctypes.c_void_p(host.data_ptr()), 1, ops.P(out), out.numel(), ops.stream())
    assert run([0, 8, 24, 32, 128, 1, 0, 0]) == 0
    assert run([0, lim["rows"] + 1, 1, 32, 128, 1, 0, 0]) == 2
    assert run([0, 8, 24, lim["oh"] + 1, 128, 1, 0, 0]) == 2
    assert run([4000, 8, 24, 32, 128, 1, 0, 0]) == 3
    assert run([0, 8, 24, 32, 128, 1, 1, 0]) == 3
    torch.cuda.synchronize()


def test_every_entry_point_through_one_ring_that_grows(dev):
    """`stack`, `windows`, `scene_windows`, `quad_windows` and `__call__` in turn through ONE collator with a ring of two slots, twice,
    the second round on larger inputs, so that the slots and the device buffer are re-allocated in the middle of the sequence: every
    result is bit for bit its host path's, and `scene_dev` holds the scene's bytes until the next call"""
    from tatt_amd import io
    LR, size = (16, 64), (64, 16)
    img = lambda seed, hs, ws, kind=None: Image.fromarray(
        R.make_image(np.random.default_rng(seed), hs, ws, seed % 3 if kind is None else kind), "RGB")
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=True, device=dev, ring=2)
    rounds = [dict(scene=img(1, 48, 160, 1), boxes=[(5, 3, 155, 17), (100, 30, 160, 48)],
                   quads=[((20, 10), (140, 30), (138, 46), (18, 26)), ((5, 26), (60, 26), (60, 46), (5, 46))],
                   lines=[img(2, 9, 40), img(3, 23, 150)], samples=R.make_batch(31, B=2)),
              dict(scene=img(4, 120, 400, 1), boxes=[(5, 3, 395, 40), (100, 60, 360, 118)],
                   quads=[((20, 10), (380, 40), (376, 76), (16, 46)), ((5, 80), (200, 80), (200, 116), (5, 116))],
                   lines=[img(5, 30, 400), img(6, 40, 600)], samples=R.make_batch(32, B=6))]
    got, caps = [], []
    for r in rounds:
        got.append(col.stack(r["lines"], size))
        caps.append(col._host[0].numel())
        got.append(col.windows(r["lines"], 32))
        caps.append(col._host[0].numel())
        for entry, what in ((col.scene_windows, r["boxes"]), (col.quad_windows, r["quads"])):
            stack, lines, scene_dev = entry(r["scene"], what, 32)
            got.append((stack, lines))
            caps.append(col._host[0].numel())
            assert np.array_equal(scene_dev.cpu().numpy(), np.asarray(r["scene"]))       # (before the next call moves the buffer on)
        got.append(col(r["samples"]))
        caps.append(col._host[0].numel())
    assert caps == sorted(caps) and len(set(caps[:5])) >= 2 and caps[5:] != [caps[4]] * 5 and len(col._host) == 2, caps
    torch.cuda.synchronize()
    for r, (stacked, (win, win_lines), (sw, sw_lines), (qw, qw_lines), batch) in zip(rounds, (got[:5], got[5:])):
        assert torch.equal(stacked.cpu(), torch.stack([io.resize_normalize(im, size, True) for im in r["lines"]]))
        want = [io.line_windows_host(im, LR, 32, True) for im in r["lines"]]
        assert torch.equal(win.cpu(), torch.cat(want)) and [len(ln.starts) for ln in win_lines] == [len(w) for w in want]
        want, lines = io.scene_windows_host(r["scene"], r["boxes"], LR, 32, True)
        assert sw_lines == lines and torch.equal(sw.cpu(), want)
        want, lines = io.quad_windows_host(r["scene"], r["quads"], LR, 32, True)
        assert qw_lines == lines and torch.equal(qw.cpu(), want)
        _same(batch, io.collate_pil_batch(r["samples"], imgH=16, imgW=64, down_sample_scale=1, mask=True, device=dev), members=(0, 2))
