"""The scene path on the GPU (csrc/scene.hip; io.DeviceCollator.scene_windows, io.DeviceExporter.scene, infer.SuperResolver.scene).
Yardstick: the host specification tatt_amd/scene.py (PIL + numpy), itself held to Pillow and to plain statements by tests/test_scene.py.
Every step around the model is integer arithmetic on uint8, so every comparison is exact (torch.equal / np.array_equal): there is no
tolerance in this file.  Shapes: the smallest at which each branch of the kernels is taken."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.fixtures import randomize_state_dict
from tests import pil_resample_ref as R

pytestmark = pytest.mark.gpu
LR = (16, 64)
STD = dict(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
# over-wide (wl = 171, five windows) | touches two scene borders, both passes skipped (64 x 16) | plain | 4 x 4 | overlaps boxes 0 and 2
BOXES = [(5, 3, 155, 17), (0, 0, 64, 16), (100, 30, 160, 48), (7, 9, 11, 13), (60, 10, 120, 40)]
DISJOINT = [(5, 3, 155, 17), (0, 20, 64, 36), (100, 30, 160, 48), (70, 20, 74, 24)]
GUARD = 0xA5


def _img(seed, hs, ws, kind=None):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, seed % 3 if kind is None else kind), "RGB")


def _diff(g, w):
    g, w = np.asarray(g), np.asarray(w)
    assert g.shape == w.shape and g.dtype == w.dtype == np.uint8, (g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), "%s: %d of %d bytes differ, max |diff| %d" % (
        g.shape, int((g != w).sum()), g.size, int(np.abs(g.astype(int) - w.astype(int)).max()))


# ---- the way in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (True, False), ids=("mask", "rgb"))
def test_scene_windows_equal_the_host_path(dev, mask):
    from tatt_amd import io
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=mask, device=dev)
    scene = _img(1, 48, 160, 1)
    want, lines = io.scene_windows_host(scene, BOXES, LR, 32, mask)
    got, got_lines, scene_dev = col.scene_windows(scene, BOXES, 32)
    assert got_lines == lines and [len(ln.starts) for ln in lines] == [5, 1, 1, 1, 1]
    assert got.shape == want.shape and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    assert scene_dev.shape == (48, 160, 3) and scene_dev.dtype == torch.uint8 and np.array_equal(scene_dev.cpu().numpy(), np.asarray(scene))
    for k, b in enumerate(BOXES):                                    # each box in a launch of its own, another stride
        g, ln, _ = col.scene_windows(scene, [b], 48)
        assert torch.equal(g.cpu(), io.line_windows_host(scene.crop(b), LR, 48, mask)), k
    empty, none, scene_dev = col.scene_windows(scene, [], 32)
    assert empty.shape == (0, 3 + mask, 16, 64) and none == [] and np.array_equal(scene_dev.cpu().numpy(), np.asarray(scene))


def test_scene_windows_of_a_box_beyond_the_line_limits(dev):
    """a crop with more rows than the window kernel resamples: resized by PIL on the host, uploaded beside the scene, cut on the device"""
    from tatt_amd import io
    lim = io.line_limits()
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=True, device=dev)
    scene = _img(2, lim["rows"] + 60, 300, 0)
    boxes = [(5, 3, 155, 17), (10, 5, 290, lim["rows"] + 45), (0, 0, 64, 16)]
    want, lines = io.scene_windows_host(scene, boxes, LR, 32, True)
    got, got_lines, _ = col.scene_windows(scene, boxes, 32)
    assert got_lines == lines and torch.equal(got.cpu(), want)


def test_windows_entry_refuses_and_a_stale_row_gives_nan(dev):
    from tatt_amd import ops
    src = torch.randint(0, 256, (48 * 160 * 3,), dtype=torch.uint8, device=dev)
    K = 4 * 16 * 64
    out = torch.zeros(3 * K, device=dev)

    def run(rows, dev_rows=None, nbytes=None):
        host = torch.tensor(rows, dtype=torch.int32)
        d = torch.tensor(dev_rows if dev_rows is not None else rows, dtype=torch.int32).to(dev)
        return ops.LIB.tatt_scene_windows(ops.P(src), src.numel() if nbytes is None else nbytes, ctypes.c_void_p(d.data_ptr()),
                                          ctypes.c_void_p(host.data_ptr()), len(rows), ops.P(out), out.numel(), ops.stream())
    row = lambda x0=0, off=0, **kw: [kw.get(k, v) for k, v in (("src", 0), ("hs", 14), ("ws", 150), ("h", 16), ("wl", 171), ("x0", x0),
                                                                 ("w", 64), ("mask", 1), ("out", off), ("pitch", 480), ("bx", 5),
                                                                 ("by", 3), ("r12", 0), ("r13", 0), ("r14", 0), ("r15", 0))]
    assert run([row()]) == 0
    assert run([row(r13=1)]) == 1 and run([row(x0=108)]) == 2 and run([row(x0=107)]) == 0
    assert run([row(bx=11)]) == 3 and run([row(by=35)]) == 3 and run([row()], nbytes=16 * 480 + 464) == 3
    assert run([row(off=2 * K + 1)]) == 3
    out.fill_(7)
    assert run([row(0, 0), row(32, K), row(107, 2 * K)], dev_rows=[row(0, 0), row(32, K, by=35), row(107, 2 * K)]) == 0
    torch.cuda.synchronize()
    got = out.view(3, 4, 16, 64).cpu()
    assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[2]).any())
    assert not bool((got[0] == 7).any()) and not bool((got[2] == 7).any())
    out.fill_(7)                                                     # planes that lie outside `out`: nothing is written
    assert run([row(0, 0)], dev_rows=[row(0, 2 * K + 1)]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def _windows_entry(dev, name, buf, rows, floats):
    """one launch of a window entry on raw descriptor rows -> its float output"""
    from tatt_amd import ops
    src = torch.from_numpy(buf).to(dev)
    host = torch.tensor(rows, dtype=torch.int32)
    desc = host.to(dev)
    out = torch.full((floats,), 7.0, device=dev)
    rc = getattr(ops.LIB, name)(ops.P(src), src.numel(), ctypes.c_void_p(desc.data_ptr()), ctypes.c_void_p(host.data_ptr()), len(rows),
                                ops.P(out), out.numel(), ops.stream())
    assert rc == 0, (name, rc)
    return out.cpu()


def _embedded(a, bx, by, pad):
    """a's pixels as the box at (bx, by) of a larger guard-filled image whose rows are `pad` bytes wider than the box's right edge"""
    hs, ws = a.shape[:2]
    pitch = 3 * (bx + ws) + pad
    buf = np.full((by + hs) * pitch, GUARD, np.uint8)
    np.lib.stride_tricks.as_strided(buf[by * pitch + 3 * bx:], a.shape, (pitch, 3, 1))[...] = a
    return buf, pitch


@pytest.mark.parametrize("mask", (True, False), ids=("mask", "rgb"))
def test_the_three_window_entries_agree(dev, mask):
    """tatt_collate_images, tatt_line_windows and tatt_scene_windows run one window body: a whole image is the window x0 = 0, w = wl, a
    box is a source with a row pitch and an origin.  Target 4 x 8; sources that take both passes, the horizontal one alone, the vertical
    one alone, neither, and a down-scale (ksize > 5).  Then three windows of one line: the two entries that cut windows, against the host"""
    from tatt_amd import io
    h, w, m = 4, 8, int(mask)
    K = (3 + m) * h * w
    for hs, ws in ((5, 7), (4, 7), (5, 8), (4, 8), (37, 50)):
        a = R.make_image(np.random.default_rng(64 * hs + ws), hs, ws, (hs + ws) % 3)
        want = io.resize_normalize(Image.fromarray(a, "RGB"), (w, h), mask).reshape(-1)
        col = _windows_entry(dev, "tatt_collate_images", a.reshape(-1), [[0, hs, ws, h, w, m, 0, 0]], K)
        lin = _windows_entry(dev, "tatt_line_windows", a.reshape(-1), [[0, hs, ws, h, w, 0, w, m, 0, 0, 0, 0]], K)
        buf, pitch = _embedded(a, 3, 2, 5)
        scw = _windows_entry(dev, "tatt_scene_windows", buf, [[0, hs, ws, h, w, 0, w, m, 0, pitch, 3, 2, 0, 0, 0, 0]], K)
        assert torch.equal(col, lin) and torch.equal(lin, scw), (hs, ws)
        assert torch.equal(col, want), (hs, ws, int((col != want).sum()))
    hs, ws, wl, starts = 5, 25, 20, (0, 6, 12)
    a = R.make_image(np.random.default_rng(9), hs, ws, 1)
    want = io.line_windows_host(Image.fromarray(a, "RGB"), (h, w), 6, mask).reshape(-1)
    assert want.numel() == 3 * K
    lin = _windows_entry(dev, "tatt_line_windows", a.reshape(-1), [[0, hs, ws, h, wl, x0, w, m, k * K, 0, 0, 0] for k, x0 in enumerate(starts)],
                         3 * K)
    buf, pitch = _embedded(a, 3, 2, 5)
    scw = _windows_entry(dev, "tatt_scene_windows", buf,
                         [[0, hs, ws, h, wl, x0, w, m, k * K, pitch, 3, 2, 0, 0, 0, 0] for k, x0 in enumerate(starts)], 3 * K)
    assert torch.equal(lin, scw) and torch.equal(lin, want), int((lin != want).sum())


# ---- the tiled resampler ------------------------------------------------------------------------------------------------------------
def _resize_cases():
    from tatt_amd import io
    lim = io.scene_limits()
    th, tw = lim["tile_h"], lim["tile_w"]
    cases = [((70, 150), (140, 300)), ((53, 131), (159, 393)), ((70, 150), (35, 75)), ((61, 97), (100, 200)), ((32, 342), (28, 300)),
             ((32, 128), (8, 40)), ((32, 128), (2, 8)), ((1, 1), (5, 7)),
             ((th + 9, tw + 5), (2 * th + 7, 2 * tw + 11)),            # three tiles per axis, a ragged last one
             ((70, 150), (70, 300)), ((70, 150), (35, 150)), ((40, 90), (40, 90)),        # a pass skipped, both skipped
             ((16 * 9, 40), (9, 40))]                                  # 16 : 1 in the vertical alone: tiles of one row
    assert -(-cases[8][1][0] // th) == 3 and -(-cases[8][1][1] // tw) == 3 and cases[8][1][0] % th and cases[8][1][1] % tw
    return cases


def _run_resize(dev, items, feather=0, old=None):
    """items: [(source array, (OH, OW))] -> (their targets cut out of the destination, the destination, the rectangles): every source
    and every target lies at a non-zero offset with a pitch wider than its rows, in buffers pre-filled with a guard byte (or `old`)"""
    from tatt_amd import ops
    rows, soff, doff, srcs, rects = [], 16, 48, [], []
    for a, (oh, ow) in items:
        hs, ws = a.shape[:2]
        sp, dp = 3 * ws + 7, 3 * ow + 13
        rows.append([soff, hs, ws, sp, doff, oh, ow, dp, feather] + [0] * 7)
        srcs.append((soff, sp, a))
        rects.append((doff, dp, oh, ow))
        soff += hs * sp + 5
        doff += oh * dp + 9
    sbuf = np.full(soff, 0x3C, np.uint8)
    for o, sp, a in srcs:
        np.lib.stride_tricks.as_strided(sbuf[o:], a.shape, (sp, 3, 1))[...] = a
    dbuf = np.full(doff, GUARD, np.uint8) if old is None else old.copy()
    s, d = torch.from_numpy(sbuf).to(dev), torch.from_numpy(dbuf).to(dev)
    host = torch.tensor(rows, dtype=torch.int32)
    desc = host.to(dev)
    rc = ops.LIB.tatt_resize_u8(ops.P(s), s.numel(), ctypes.c_void_p(desc.data_ptr()), ctypes.c_void_p(host.data_ptr()), len(rows), ops.P(d),
                                d.numel(), ops.stream())
    assert rc == 0, rc
    out = d.cpu().numpy()
    return [np.lib.stride_tricks.as_strided(out[o:], (oh, ow, 3), (dp, 3, 1)).copy() for o, dp, oh, ow in rects], out, rects, dbuf


def _outside(out, rects, before):
    """every byte outside the target rectangles is what it was"""
    keep = np.ones(out.size, bool)
    for o, dp, oh, ow in rects:
        for y in range(oh):
            keep[o + y * dp:o + y * dp + 3 * ow] = False
    return np.array_equal(out[keep], before[keep])


def test_resize_equals_pillow_in_one_launch_and_alone(dev):
    cases = _resize_cases()
    srcs = [R.make_image(np.random.default_rng(30 + i), hs, ws, i % 3) for i, ((hs, ws), _) in enumerate(cases)]
    want = [np.asarray(Image.fromarray(a, "RGB").resize((ow, oh), Image.BICUBIC)) for a, (_, (oh, ow)) in zip(srcs, cases)]
    got, out, rects, before = _run_resize(dev, [(a, c[1]) for a, c in zip(srcs, cases)])      # all items in one launch
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (cases[i], int((g != w).sum()), g.size)
    assert _outside(out, rects, before)
    for i in (0, 6, 7, 8):                                           # alone: the grid and the LDS are sized by this item
        got, out, rects, before = _run_resize(dev, [(srcs[i], cases[i][1])])
        assert np.array_equal(got[0], want[i]) and _outside(out, rects, before), cases[i]


@pytest.mark.parametrize("feather", (1, 3, 40))
def test_resize_feathers_into_what_the_target_holds(dev, feather):
    rng = np.random.default_rng(feather)
    items = [(R.make_image(rng, 32, 128, 1), (50, 161)), (R.make_image(rng, 32, 342, 0), (28, 300)), (R.make_image(rng, 9, 9, 1), (9, 9))]
    old = rng.integers(0, 256, 48 + sum(oh * (3 * ow + 13) + 9 for _, (oh, ow) in items), dtype=np.uint8)
    got, out, rects, before = _run_resize(dev, items, feather, old)
    D = feather + 1
    for (a, (oh, ow)), g, (o, dp, _, _) in zip(items, got, rects):
        new = np.asarray(Image.fromarray(a, "RGB").resize((ow, oh), Image.BICUBIC)).astype(np.int64)
        was = np.lib.stride_tricks.as_strided(old[o:], (oh, ow, 3), (dp, 3, 1)).astype(np.int64)
        i, j = np.arange(oh)[:, None], np.arange(ow)[None, :]
        w = np.minimum(np.minimum(np.minimum(i, oh - 1 - i), np.minimum(j, ow - 1 - j)) + 1, D)[:, :, None]
        assert np.array_equal(g, ((2 * (w * new + (D - w) * was) + D) // (2 * D)).astype(np.uint8))
    assert _outside(out, rects, before)


def test_resize_entry_refuses_and_a_stale_row_writes_nothing(dev):
    from tatt_amd import io, ops
    lim = io.scene_limits()
    src = torch.randint(0, 256, (70 * 450,), dtype=torch.uint8, device=dev)
    dst = torch.full((16 + 140 * 912,), 7, dtype=torch.uint8, device=dev)

    def run(row, dev_row=None, sb=None, db=None):
        host = torch.tensor([row], dtype=torch.int32)
        d = torch.tensor([dev_row if dev_row is not None else row], dtype=torch.int32).to(dev)
        return ops.LIB.tatt_resize_u8(ops.P(src), src.numel() if sb is None else sb, ctypes.c_void_p(d.data_ptr()),
                                      ctypes.c_void_p(host.data_ptr()), 1, ops.P(dst), dst.numel() if db is None else db, ops.stream())
    row = lambda **kw: [kw.get(k, v) for k, v in (("src", 0), ("hs", 70), ("ws", 150), ("sp", 450), ("dst", 16), ("oh", 140), ("ow", 300),
                                                  ("dp", 912), ("f", 0))] + [kw.get("r%d" % i, 0) for i in range(9, 16)]
    assert run(row(r9=1)) == 1 and run(row(f=-1)) == 1
    assert run(row(oh=4)) == 2 and run(row(ow=9)) == 2 and run(row(f=lim["feather"] + 1)) == 2
    assert run(row(src=1)) == 3 and run(row(sp=449)) == 3 and run(row(dst=32)) == 3 and run(row(dp=899)) == 3 and run(row(), db=100) == 3
    for stale in (row(r12=1), row(ow=9), row(src=1), row(dst=32), row(dp=899), row(f=-2)):
        assert run(row(), dev_row=stale) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7).all())
    assert run(row()) == 0
    torch.cuda.synchronize()
    assert bool((dst[:16] == 7).all()) and not bool((dst[16:916] == 7).all())


# ---- the pastes ---------------------------------------------------------------------------------------------------------------------
def _sr_stack(lines, seed):
    """an SR stack like a generator's output, with values below 0 and above 1"""
    n = lines[-1].first + len(lines[-1].starts)
    return torch.rand(n, 4, 32, 128, generator=torch.Generator().manual_seed(seed)) * 1.4 - 0.2


@pytest.mark.parametrize("feather", (0, 3))
@pytest.mark.parametrize("boxes", (DISJOINT, BOXES), ids=("disjoint", "layers"))
def test_paste_equals_the_host_composition(dev, boxes, feather):
    from tatt_amd import io
    scene = _img(4, 48, 160, 0)
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=True, device=dev)
    ex = io.DeviceExporter(device=dev, rule="floor")
    _, lines, scene_dev = col.scene_windows(scene, boxes, 32)
    assert max(io.scene_layers(boxes)) == (0 if boxes is DISJOINT else 2)
    sr = _sr_stack(lines, len(boxes))
    calls = []
    from tatt_amd import ops
    real = ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        pending = ex.scene(scene_dev, sr.to(dev), lines, boxes, 2, feather)
    finally:
        ops.call = real
    assert calls == ["tatt_line_blend"] + ["tatt_resize_u8"] * (2 if boxes is DISJOINT else 4)
    got = pending.result()
    assert len(got) == 1 and got[0].size == (320, 96) and got[0].mode == "RGB"
    imgs = [io.blend_windows_host(sr[ln.first:ln.first + len(ln.starts)], ln.starts, ln.wl, 2, "floor") for ln in lines]
    _diff(got[0], io.scene_compose_host(scene, boxes, imgs, 2, feather))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _generator(dev, cls="TSRN", seed=1234):
    import tatt_amd
    torch.manual_seed(seed)
    m = getattr(tatt_amd, cls)(**STD)
    m.load_state_dict(randomize_state_dict(m.state_dict()))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def tsrn_scene(dev):
    from tatt_amd.infer import SuperResolver
    up = SuperResolver(_generator(dev), batch_size=4, lr_size=LR, mask=True, rule="floor", keep_sr=True, stride=32)
    scene = _img(60, 48, 160, 1)
    pending = up.scene(scene, BOXES, 3)
    return up, scene, pending, pending.result()


def _check_against_host(io, scene, boxes, feather, pending, image):
    want_lr, lines = io.scene_windows_host(scene, boxes, LR, 32, True)
    assert pending.lines == lines and pending.boxes == boxes and pending.layers == io.scene_layers(boxes)
    assert torch.equal(pending.lr.cpu(), want_lr)
    sr = pending.sr.cpu()
    assert sr.shape == (want_lr.shape[0], sr.shape[1], 32, 128)
    rows = iter(sr.split([len(ln.starts) for ln in lines]))
    assert image.mode == "RGB" and image.size == (2 * scene.size[0], 2 * scene.size[1])
    _diff(image, io.super_resolve_scene_host(scene, boxes, lambda x: next(rows), LR, 32, True, "floor", feather=feather))


def test_super_resolver_scene_equals_the_host_composition_of_its_own_sr(dev, tsrn_scene):
    from tatt_amd import io
    up, scene, pending, image = tsrn_scene
    assert pending.lr.shape[0] == 9 and sorted(up.sessions) == [1, 4]             # nine windows at batch_size 4: 4 + 4 + 1
    _check_against_host(io, scene, BOXES, 3, pending, image)


def test_scene_without_boxes_is_the_plain_upscale(dev, tsrn_scene):
    up, scene, _, _ = tsrn_scene
    n = len(up.sessions)
    p = up.scene(scene, [])
    _diff(p.result(), scene.resize((320, 96), Image.BICUBIC))
    assert p.sr is None and p.lines == [] and p.boxes == [] and p.layers == [] and len(up.sessions) == n
    big = _img(61, 141, 333, 0)                                       # several tiles per axis, ragged
    _diff(up.scene(big, []).result(), big.resize((666, 282), Image.BICUBIC))


def test_second_scene_call_makes_no_host_wait_before_result(dev, tsrn_scene):
    from tatt_amd import io
    up, scene, pending, image = tsrn_scene
    again = _img(62, 48, 160, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = up.scene(again, BOXES, 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check_against_host(io, again, BOXES, 0, p, p.result())
    _diff(up.scene(scene, BOXES, 3).result(), image)                 # and the first scene gives its bytes again


def test_tatt_generator_scene_on_the_zero_prior(dev):
    from tatt_amd import io
    from tatt_amd.infer import SuperResolver
    up = SuperResolver(_generator(dev, "TSRN_TL_TRANS"), batch_size=4, lr_size=LR, mask=True, rule="floor", keep_sr=True)
    scene = _img(63, 48, 160, 1)
    boxes = [(20, 4, 130, 20), (0, 30, 40, 44)]                       # wl = 110: 3 windows, + 1: one session of 4
    p = up.scene(scene, boxes, 1)
    image = p.result()
    assert sorted(up.sessions) == [4]
    _check_against_host(io, scene, boxes, 1, p, image)


def test_scene_refuses_a_recogniser_a_bad_stride_and_bad_boxes(dev, tsrn_scene):
    import tatt_amd
    from tatt_amd.infer import SuperResolver
    up, scene, _, _ = tsrn_scene
    rec = tatt_amd.CRNN(32, 1, 37, 256).to(dev).eval()
    with pytest.raises(ValueError, match="recogni"):
        SuperResolver(up.gen, recognizer=rec).scene(scene, BOXES)
    with pytest.raises(ValueError, match="stride"):
        SuperResolver(up.gen, stride=16).scene(scene, BOXES)
    for bad in ((0, 0, 3, 16), (100, 0, 161, 16), (8, 0, 8, 16), (0.0, 0, 8, 16)):
        with pytest.raises(ValueError, match="box 0"):
            up.scene(scene, [bad])
    with pytest.raises(ValueError, match="feather"):
        up.scene(scene, BOXES, -1)


# ---- untouched paths ----------------------------------------------------------------------------------------------------------------
def test_crops_and_long_lines_give_the_bytes_of_their_host_yardsticks(dev, tsrn_scene):
    from tatt_amd import io
    from tatt_amd.infer import SuperResolver
    gen = tsrn_scene[0].gen
    crops = [_img(80 + i, hs, ws) for i, (hs, ws) in enumerate(((16, 64), (23, 90), (9, 40)))]
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, mask=True, rule="floor", keep_sr=True)
    p = plain(crops)
    got = p.result()
    assert len(p.sr) == 1 and sorted(plain.sessions) == [3]
    for g, w in zip(got, io.export_pil_batch(p.sr[0].cpu(), None, "floor")):
        _diff(g, w)
    lr = torch.stack([io.resize_normalize(im, (64, 16), True) for im in crops])          # the session read the host yardstick's bytes
    assert torch.equal(plain.sessions[3].run(lr.to(dev))[0].cpu(), p.sr[0].cpu())
    long = SuperResolver(gen, batch_size=4, lr_size=LR, mask=True, rule="floor", keep_sr=True, long_lines=True)
    lines_in = [_img(90, 23, 301), _img(91, 16, 64)]
    p = long(lines_in)
    got = p.result()
    assert torch.equal(p.lr.cpu(), torch.cat([io.line_windows_host(im, LR, 32, True) for im in lines_in]))
    rows = iter(p.sr.cpu().split([len(ln.starts) for ln in p.lines]))
    for g, w in zip(got, io.super_resolve_lines_host(lines_in, lambda x: next(rows), LR, 32, True, "floor")):
        _diff(g, w)
