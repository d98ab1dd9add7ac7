"""Quadrilateral text boxes on the GPU (csrc/quads.hip; io.DeviceCollator.quad_windows, io.DeviceExporter.scene_quads,
infer.SuperResolver.scene_quads).  Yardstick: the host specification tatt_amd/quads.py (numpy int64 + PIL), itself held to an independent
scalar restatement by tests/test_quads.py.  Every step around the model is integer arithmetic on uint8, so every comparison is exact
(torch.equal / np.array_equal): there is no tolerance in this file.  Shapes: the smallest at which each branch of the kernel is taken."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.fixtures import randomize_state_dict
from tests import pil_resample_ref as R

pytestmark = pytest.mark.gpu
LR = (16, 64)
STD = dict(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
ONE = ((150, 60), (200, 62), (199, 88), (149, 86))                   # one window
THREE = ((20, 10), (140, 30), (138, 46), (18, 26))                   # 122 x 16 rectified: wl = 122, three windows
PERSX = ((30, 10), (180, 25), (175, 70), (35, 90))                   # perspective; its bounding box meets THREE's
AXIS = ((5, 60), (60, 60), (60, 80), (5, 80))
QUADS = [ONE, THREE, PERSX]                                          # 1 + 3 + 1 windows: at batch_size 3 a batch ends inside THREE's line
DISJOINT = [ONE, THREE, AXIS]
GUARD = 0xA5


def _img(seed, hs, ws, kind=None):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, seed % 3 if kind is None else kind), "RGB")


def _diff(g, w):
    g, w = np.asarray(g), np.asarray(w)
    assert g.shape == w.shape and g.dtype == w.dtype == np.uint8, (g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), "%s: %d of %d bytes differ, max |diff| %d" % (
        g.shape, int((g != w).sum()), g.size, int(np.abs(g.astype(int) - w.astype(int)).max()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def warp_items():
    """[(source, matrix, OH, OW, mode, feather)]: identity, rotated and perspective matrices; destination heights and widths 1, tile - 1,
    tile, tile + 1; both modes; feather 0, 1 and 5"""
    from tatt_amd import io
    lim = io.quad_limits()
    th, tw = lim["tile_h"], lim["tile_w"]
    src = R.make_image(np.random.default_rng(40), 40, 90, 1)
    one = 1 << io.QUAD_SHIFT
    ident = (one // 2, 0, 0, 0, one // 2, 0, 0, 0, one)
    rot = ((10, 4), (80, 16), (76, 36), (6, 24))
    per = ((8, 5), (80, 12), (76, 36), (10, 30))
    io.quad_check((90, 40), [rot, per])
    mats = [(ident, ident)] + [io.quad_matrices(q, 1)[:2] for q in (rot, per)]
    sizes = list(itertools.product((1, th - 1, th, th + 1), (1, tw - 1, tw, tw + 1)))
    items = []
    for n, (oh, ow) in enumerate(sizes):
        m_r, m_p = mats[n % 3]
        mode = (n // 3) % 2
        items.append((src, m_p if mode else m_r, oh, ow, mode, (0, 1, 5)[n % 3] if mode else 0))
    for k, (m_r, m_p) in enumerate(mats):                            # every matrix in both modes over several tiles, every feather
        items.append((src, m_r, 2 * th + 3, 2 * tw + 5, 0, 0))
        for f in (0, 1, 5):
            items.append((src, m_p, 3 * th + 1, 2 * tw + 7, 1, f))
    return items


def warp_layout(items, seed=1):
    """-> (the rows, the source buffer, the destination before the launch, [(offset, pitch, OH, OW)]): every source and every target lies
    at a non-zero offset with a pitch wider than its rows"""
    from tatt_amd.quads import warp_row
    rows, soff, doff, srcs, rects = [], 16, 48, [], []
    for a, m, oh, ow, mode, f in items:
        hs, ws = a.shape[:2]
        sp, dp = 3 * ws + 7, 3 * ow + 13
        rows.append(warp_row(soff, hs, ws, sp, doff, oh, ow, dp, f, mode, m))
        srcs.append((soff, sp, a))
        rects.append((doff, dp, oh, ow))
        soff += hs * sp + 5
        doff += oh * dp + 9
    sbuf = np.full(soff, 0x3C, np.uint8)
    for o, sp, a in srcs:
        np.lib.stride_tricks.as_strided(sbuf[o:], a.shape, (sp, 3, 1))[...] = a
    before = np.random.default_rng(seed).integers(0, 256, doff, dtype=np.uint8)
    return np.array(rows, np.int32), sbuf, before, rects


def warp_wants(items, before, rects):
    """what the host yardstick makes of every target, and the mask of the bytes outside all targets"""
    from tatt_amd import io
    want, keep = [], np.ones(before.size, bool)
    for (a, m, oh, ow, mode, f), (o, dp, _, _) in zip(items, rects):
        old = np.lib.stride_tricks.as_strided(before[o:], (oh, ow, 3), (dp, 3, 1)).copy()
        want.append(io.warp_u8_host(a, m, oh, ow, old, f) if mode else io.warp_u8_host(a, m, oh, ow))
        for y in range(oh):
            keep[o + y * dp:o + y * dp + 3 * ow] = False
    return want, keep


def _run_warp(dev, items, seed=1):
    """-> (the targets cut out of the destination, what the host yardstick makes of them, whether every byte outside the targets kept its
    value)"""
    from tatt_amd import ops
    rows, sbuf, before, rects = warp_layout(items, seed)
    s, d = torch.from_numpy(sbuf).to(dev), torch.from_numpy(before).to(dev)
    host = torch.from_numpy(rows)
    desc = host.to(dev)
    rc = ops.LIB.tatt_warp_u8(ops.P(s), s.numel(), ctypes.c_void_p(desc.data_ptr()), ctypes.c_void_p(host.data_ptr()), len(rows), ops.P(d),
                              d.numel(), ops.stream())
    assert rc == 0, rc
    out = d.cpu().numpy()
    want, keep = warp_wants(items, before, rects)
    got = [np.lib.stride_tricks.as_strided(out[o:], (oh, ow, 3), (dp, 3, 1)).copy() for o, dp, oh, ow in rects]
    return got, want, np.array_equal(out[keep], before[keep])


def test_warp_equals_the_host_yardstick_in_one_launch_and_alone(dev):
    from tatt_amd import io
    items = warp_items()
    got, want, outside = _run_warp(dev, items)                       # all items in one launch
    for n, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (n, items[n][2:], int((g != w).sum()), g.size)
    assert outside
    painted = [io.warp_inside_host(it[1], it[2], it[3], 40, 90).mean() for it in items if it[4] == 1 and it[2] > 8]
    assert min(painted) < 1 and max(painted) > 0.2                   # the pastes both paint and skip pixels
    for n, it in enumerate(items):                                   # alone: the grid is sized by this item
        got, want, outside = _run_warp(dev, [it], seed=2 + n)
        assert np.array_equal(got[0], want[0]) and outside, (n, it[2:])


def test_warp_entry_refuses_and_a_stale_row_writes_nothing(dev):
    from tatt_amd import io, ops
    from tatt_amd.quads import warp_row
    lim = io.quad_limits()
    src = torch.randint(0, 256, (70 * 450,), dtype=torch.uint8, device=dev)
    dst = torch.full((16 + 140 * 912,), 7, dtype=torch.uint8, device=dev)
    one = 1 << io.QUAD_SHIFT
    m = (one // 4, 0, 0, 0, one // 4, 0, 0, 0, one)

    def row(**kw):
        base = dict(src=0, hs=70, ws=150, sp=450, dst=16, oh=140, ow=300, dp=912, f=0, mode=0)
        base.update({k: v for k, v in kw.items() if k in base})
        r = warp_row(*(base[k] for k in ("src", "hs", "ws", "sp", "dst", "oh", "ow", "dp", "f", "mode")), m)
        for i in range(28, 32):
            r[i] = kw.get("r%d" % i, 0)
        return r

    def run(r, dev_row=None, sb=None, db=None):
        host = torch.tensor([r], dtype=torch.int32)
        d = torch.tensor([dev_row if dev_row is not None else r], dtype=torch.int32).to(dev)
        return ops.LIB.tatt_warp_u8(ops.P(src), src.numel() if sb is None else sb, ctypes.c_void_p(d.data_ptr()),
                                    ctypes.c_void_p(host.data_ptr()), 1, ops.P(dst), dst.numel() if db is None else db, ops.stream())
    assert run(row(r29=1)) == 1 and run(row(f=-1)) == 1 and run(row(mode=3)) == 1
    assert run(row(oh=lim["side"] + 1)) == 2 and run(row(f=lim["feather"] + 1)) == 2 and run(row(ws=0)) == 2
    assert run(row(src=1)) == 3 and run(row(sp=449)) == 3 and run(row(dst=32)) == 3 and run(row(dp=899)) == 3 and run(row(), db=100) == 3
    for stale in (row(r30=1), row(mode=2), row(src=1), row(dst=32), row(dp=899), row(f=-2), row(ow=lim["side"] + 1)):
        assert run(row(), dev_row=stale) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7).all())
    assert run(row()) == 0
    torch.cuda.synchronize()
    assert bool((dst[:16] == 7).all()) and not bool((dst[16:916] == 7).all())


# ---- the way in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (True, False), ids=("mask", "rgb"))
def test_quad_windows_equal_the_host_path(dev, mask):
    from tatt_amd import io
    lim = io.line_limits()
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=mask, device=dev)
    scene = _img(1, 97, 211, 1)
    want, lines = io.quad_windows_host(scene, QUADS, LR, 32, mask)
    got, got_lines, scene_dev = col.quad_windows(scene, QUADS, 32)
    assert got_lines == lines and [len(ln.starts) for ln in lines] == [1, 3, 1]
    assert got.shape == want.shape and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    assert scene_dev.shape == (97, 211, 3) and scene_dev.dtype == torch.uint8 and np.array_equal(scene_dev.cpu().numpy(), np.asarray(scene))
    empty, none, scene_dev = col.quad_windows(scene, [], 32)
    assert empty.shape == (0, 3 + mask, 16, 64) and none == [] and np.array_equal(scene_dev.cpu().numpy(), np.asarray(scene))
    # a crop taller than the window kernel resamples (16-row windows: beyond the tiled resampler's 16 : 1 too -> the uploaded fallback)
    tall = lim["rows"] + 20
    scene = _img(2, tall + 30, 300, 0)
    quads = [((150, 60), (200, 62), (199, 88), (149, 86)), ((20, 10), (140, 30), (138, 46), (18, 26)),
             ((10, 5), (290, 8), (288, tall + 10), (12, tall + 5))]
    want, lines = io.quad_windows_host(scene, quads, LR, 32, mask)
    got, got_lines, _ = col.quad_windows(scene, quads, 32)
    assert io.quad_size(quads[2])[1] > lim["rows"] and got_lines == lines and torch.equal(got.cpu(), want)


def test_quad_windows_resize_a_crop_beyond_the_line_limits_on_the_device(dev):
    """32-row windows: the tall crop shrinks by less than 16 : 1, so ONE tatt_resize_u8 launch makes its (wl, 32) version on the device"""
    from tatt_amd import io, ops
    lim = io.line_limits()
    tall = lim["rows"] + 20
    col = io.DeviceCollator(imgH=32, imgW=128, down_sample_scale=1, mask=True, device=dev)
    scene = _img(3, tall + 30, 300, 1)
    quads = [((150, 60), (200, 62), (199, 88), (149, 86)), ((10, 5), (290, 8), (288, tall + 10), (12, tall + 5)),
             ((20, 10), (140, 30), (138, 46), (18, 26))]
    want, lines = io.quad_windows_host(scene, quads, (32, 128), 64, True)
    calls, real = [], ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        got, got_lines, _ = col.quad_windows(scene, quads, 64)
    finally:
        ops.call = real
    assert calls == ["tatt_warp_u8", "tatt_resize_u8", "tatt_scene_windows"]
    assert got_lines == lines and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())


# ---- the pastes ---------------------------------------------------------------------------------------------------------------------
def _sr_stack(lines, seed):
    """an SR stack like a generator's output, with values below 0 and above 1"""
    n = lines[-1].first + len(lines[-1].starts)
    return torch.rand(n, 4, 32, 128, generator=torch.Generator().manual_seed(seed)) * 1.4 - 0.2


@pytest.mark.parametrize("feather", (0, 2))
@pytest.mark.parametrize("quads", (DISJOINT, QUADS), ids=("disjoint", "layers"))
def test_scene_quads_export_equals_the_host_composition(dev, quads, feather):
    from tatt_amd import io, ops
    scene = _img(4, 97, 211, 0)
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=True, device=dev)
    ex = io.DeviceExporter(device=dev, rule="floor")
    _, lines, scene_dev = col.quad_windows(scene, quads, 32)
    n_layers = 1 + max(io.quad_layers(quads))
    assert n_layers == (1 if quads is DISJOINT else 2)
    sr = _sr_stack(lines, len(quads))
    calls, real = [], ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        pending = ex.scene_quads(scene_dev, sr.to(dev), lines, quads, 2, feather)
    finally:
        ops.call = real
    assert calls == ["tatt_line_blend", "tatt_resize_u8", "tatt_resize_u8"] + ["tatt_warp_u8"] * n_layers
    got = pending.result()
    assert len(got) == 1 and got[0].size == (422, 194) and got[0].mode == "RGB"
    imgs = [io.blend_windows_host(sr[ln.first:ln.first + len(ln.starts)], ln.starts, ln.wl, 2, "floor") for ln in lines]
    _diff(got[0], io.quad_compose_host(scene, quads, imgs, 2, feather))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _generator(dev, cls="TSRN", seed=1234):
    import tatt_amd
    torch.manual_seed(seed)
    m = getattr(tatt_amd, cls)(**STD)
    m.load_state_dict(randomize_state_dict(m.state_dict()))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def tsrn_quads(dev):
    from tatt_amd.infer import SuperResolver
    up = SuperResolver(_generator(dev), batch_size=3, lr_size=LR, mask=True, rule="floor", keep_sr=True, stride=32)
    scene = _img(60, 97, 211, 1)
    pending = up.scene_quads(scene, QUADS, 3)
    return up, scene, pending, pending.result()


def _check_against_host(io, scene, quads, feather, pending, image):
    want_lr, lines = io.quad_windows_host(scene, quads, LR, 32, True)
    assert pending.lines == lines and pending.boxes == quads and pending.layers == io.quad_layers(quads)
    assert torch.equal(pending.lr.cpu(), want_lr)
    sr = pending.sr.cpu()
    assert sr.shape == (want_lr.shape[0], sr.shape[1], 32, 128)
    rows = iter(sr.split([len(ln.starts) for ln in lines]))
    assert image.mode == "RGB" and image.size == (2 * scene.size[0], 2 * scene.size[1])
    _diff(image, io.super_resolve_quads_host(scene, quads, lambda x: next(rows), LR, 32, True, "floor", feather=feather))


def test_super_resolver_scene_quads_equals_the_host_composition_of_its_own_sr(dev, tsrn_quads):
    from tatt_amd import io
    up, scene, pending, image = tsrn_quads
    assert pending.lr.shape[0] == 5 and sorted(up.sessions) == [2, 3]              # five windows at batch_size 3: 3 + 2
    _check_against_host(io, scene, QUADS, 3, pending, image)
    assert not np.array_equal(np.asarray(image), np.asarray(scene.resize((422, 194), Image.BICUBIC)))


@pytest.mark.parametrize("feather", (0, 2))
def test_axis_aligned_quads_give_the_bytes_of_scene_on_the_boxes(dev, tsrn_quads, feather):
    up, scene, _, _ = tsrn_quads
    boxes = [(20, 10, 170, 40), (100, 30, 200, 70), (5, 50, 25, 60)]                       # the first two overlap
    quads = [((x0, y0), (x1, y0), (x1, y1), (x0, y1)) for x0, y0, x1, y1 in boxes]
    a = up.scene_quads(scene, quads, feather)
    b = up.scene(scene, boxes, feather)
    assert torch.equal(a.lr, b.lr) and a.lines == b.lines
    _diff(a.result(), b.result())


def test_scene_quads_without_quads_is_the_plain_upscale(dev, tsrn_quads):
    up, scene, _, _ = tsrn_quads
    n = len(up.sessions)
    p = up.scene_quads(scene, [])
    _diff(p.result(), scene.resize((422, 194), Image.BICUBIC))
    assert p.sr is None and p.lines == [] and p.boxes == [] and p.layers == [] and len(up.sessions) == n


def test_second_scene_quads_call_makes_no_host_wait_before_result(dev, tsrn_quads):
    from tatt_amd import io
    up, scene, pending, image = tsrn_quads
    again = _img(62, 97, 211, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = up.scene_quads(again, QUADS, 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check_against_host(io, again, QUADS, 0, p, p.result())
    _diff(up.scene_quads(scene, QUADS, 3).result(), image)           # and the first scene gives its bytes again


def test_tatt_generator_scene_quads_on_the_zero_prior(dev):
    from tatt_amd import io
    from tatt_amd.infer import SuperResolver
    up = SuperResolver(_generator(dev, "TSRN_TL_TRANS"), batch_size=3, lr_size=LR, mask=True, rule="floor", keep_sr=True)
    scene = _img(63, 97, 211, 1)
    quads = [THREE, ONE]                                             # 3 + 1 windows: sessions of 3 and 1
    p = up.scene_quads(scene, quads, 1)
    image = p.result()
    assert sorted(up.sessions) == [1, 3]
    _check_against_host(io, scene, quads, 1, p, image)


def test_scene_quads_refuses_a_recogniser_a_bad_stride_and_bad_quads(dev, tsrn_quads):
    import tatt_amd
    from tatt_amd.infer import SuperResolver
    up, scene, _, _ = tsrn_quads
    rec = tatt_amd.CRNN(32, 1, 37, 256).to(dev).eval()
    with pytest.raises(ValueError, match="recogni"):
        SuperResolver(up.gen, recognizer=rec).scene_quads(scene, QUADS)
    with pytest.raises(ValueError, match="stride"):
        SuperResolver(up.gen, stride=16).scene_quads(scene, QUADS)
    for bad in (ONE[::-1], (0, 0, 64, 16), ((150, 60), (212, 62), (199, 88), (149, 86)), ((150, 60), (200.0, 62), (199, 88), (149, 86)),
                ((20, 10), (120, 10), (120, 30), (20, 51))):
        with pytest.raises(ValueError, match="quad 0"):
            up.scene_quads(scene, [bad])
    with pytest.raises(ValueError, match="feather"):
        up.scene_quads(scene, QUADS, -1)
