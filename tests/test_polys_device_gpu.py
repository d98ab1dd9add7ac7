"""Polygon text instances, curved text, on the GPU (csrc/polys.hip; io.DeviceCollator.poly_windows, io.DeviceExporter.scene_polys,
infer.SuperResolver.scene_polys).  Yardstick: the host specification tatt_amd/polys.py (numpy int64 + PIL), itself held to exact
geometry and to the quad path by tests/test_polys.py.  Every step around the model is integer arithmetic on uint8, so every comparison
is exact (torch.equal / np.array_equal): there is no tolerance in this file.  Scenes of 96 x 200; shapes: the smallest at which each
branch of the kernel is taken."""
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
HS, WS = 96, 200
STD = dict(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
ONE = ((150, 60), (200, 62), (199, 88), (149, 86))                   # the quads of tests/test_quads_device_gpu.py: N = 2
THREE = ((20, 10), (140, 30), (138, 46), (18, 26))
PERSX = ((30, 10), (180, 25), (175, 70), (35, 90))
ARC = ((10, 40), (40, 22), (75, 18), (110, 30), (104, 50), (74, 38), (44, 42), (20, 58))                               # N = 4
SCURVE = ((10, 30), (45, 20), (85, 28), (125, 40), (165, 34), (168, 52), (123, 58), (82, 46), (47, 39), (14, 48))      # N = 5
ARC8 = ((20, 35), (41, 23), (64, 15), (88, 11), (112, 11), (136, 15), (159, 23), (180, 35),                            # N = 8
        (168, 53), (150, 43), (131, 36), (110, 32), (90, 32), (69, 36), (50, 43), (32, 53))
RECT3 = ((120, 5), (132, 5), (150, 5), (150, 13), (132, 13), (120, 13))                  # N = 3, axis-aligned: every pixel of its box
POLYS = [ONE, ARC, SCURVE]                                           # 1 + 2 + 4 windows; SCURVE's bounding box meets ARC's: two layers
DISJOINT = [ARC, ONE, RECT3]


def _tiny(w, h, x=60, y=70):
    """N = 4 with a bounding box of exactly w x h: two slanted end strips of 10 columns around a rectangle"""
    return ((x, y + 2), (x + 10, y), (x + w - 10, y), (x + w, y + 2), (x + w, y + h), (x + w - 10, y + h - 2), (x + 10, y + h - 2), (x, y + h))


def _img(seed, hs, ws, kind=None):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, seed % 3 if kind is None else kind), "RGB")


def _diff(g, w):
    g, w = np.asarray(g), np.asarray(w)
    assert g.shape == w.shape and g.dtype == w.dtype == np.uint8, (g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), "%s: %d of %d bytes differ, max |diff| %d" % (
        g.shape, int((g != w).sum()), g.size, int(np.abs(g.astype(int) - w.astype(int)).max()))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def paste_items():
    """[(line, maps, OH, OW, feather)]: bounding boxes of tile - 1, tile and tile + 1 rows and columns (N = 4), targets of 1 row or 1
    column (the corner of an axis-aligned N = 3 polygon: the check wants four rows and two columns per strip, so no true box is that
    small), then N = 2, 4, 5 and 8 over their whole boxes at scale 1 and 2 with feather 0, 1 and 5"""
    from tatt_amd import io
    lim = io.poly_limits()
    th, tw = lim["tile_h"], lim["tile_w"]
    rng = np.random.default_rng(40)
    items = []

    def add(poly, scale, feather, oh=None, ow=None):
        io.poly_check((WS, HS), [poly])
        maps = io.poly_matrices(poly, scale)
        bw, bh = io.poly_size(poly)
        x0, y0, x1, y1 = maps.bbox
        line = R.make_image(rng, scale * bh, scale * bw, len(items) % 3)
        items.append((line, maps, scale * (y1 - y0) if oh is None else oh, scale * (x1 - x0) if ow is None else ow, feather))
    for n, (oh, ow) in enumerate(itertools.product((1, th - 1, th, th + 1), (1, tw - 1, tw, tw + 1))):
        if oh == 1 or ow == 1:
            add(RECT3, 1, (0, 1, 5)[n % 3], oh, ow)
        else:
            add(_tiny(ow, oh), 1, (0, 1, 5)[n % 3])
    for poly in (THREE, ARC, SCURVE, ARC8):
        for scale in (1, 2):
            for feather in (0, 1, 5):
                add(poly, scale, feather)
    return items


def paste_layout(items, seed=1):
    """-> (item rows, strip rows, the line buffer, the destination before the launch, [(offset, pitch, OH, OW)]): every line and every
    target lies at a non-zero offset with a pitch wider than its rows; one strip table for all items"""
    from tatt_amd.polys import poly_item_row, poly_strip_row
    rows, strips, soff, doff, srcs, rects = [], [], 16, 48, [], []
    for line, maps, oh, ow, f in items:
        hs, ws = line.shape[:2]
        sp, dp = 3 * ws + 7, 3 * ow + 13
        rows.append(poly_item_row(soff, hs, ws, sp, doff, oh, ow, dp, f, len(strips), len(maps.paste)))
        start, last = 0, len(maps.paste) - 1
        for k, m in enumerate(maps.paste):
            strips.append(poly_strip_row(maps.scale * start, maps.scale * maps.widths[k], m, maps.seams[k - 1] if k else None,
                                         maps.seams[k] if k < last else None))
            start += maps.widths[k]
        srcs.append((soff, sp, line))
        rects.append((doff, dp, oh, ow))
        soff += hs * sp + 5
        doff += oh * dp + 9
    sbuf = np.full(soff, 0x3C, np.uint8)
    for o, sp, a in srcs:
        np.lib.stride_tricks.as_strided(sbuf[o:], a.shape, (sp, 3, 1))[...] = a
    before = np.random.default_rng(seed).integers(0, 256, doff, dtype=np.uint8)
    return np.array(rows, np.int32), np.array(strips, np.int32), sbuf, before, rects


def paste_wants(items, before, rects):
    """what the host yardstick makes of every target, and the mask of the bytes outside all targets"""
    from tatt_amd import io
    want, keep = [], np.ones(before.size, bool)
    for (line, maps, oh, ow, f), (o, dp, _, _) in zip(items, rects):
        old = np.lib.stride_tricks.as_strided(before[o:], (oh, ow, 3), (dp, 3, 1)).copy()
        want.append(io.poly_paste_host(line, maps, old, f))
        for y in range(oh):
            keep[o + y * dp:o + y * dp + 3 * ow] = False
    return want, keep


def _run_paste(dev, items, seed=1):
    from tatt_amd import ops
    rows, strips, sbuf, before, rects = paste_layout(items, seed)
    s, d = torch.from_numpy(sbuf).to(dev), torch.from_numpy(before).to(dev)
    hrows, hstrips = torch.from_numpy(rows), torch.from_numpy(strips)
    drows, dstrips = hrows.to(dev), hstrips.to(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = ops.LIB.tatt_poly_paste_u8(P(s), s.numel(), P(drows), P(hrows), len(rows), P(dstrips), P(hstrips), len(strips), P(d), d.numel(),
                                    ops.stream())
    assert rc == 0, rc
    out = d.cpu().numpy()
    want, keep = paste_wants(items, before, rects)
    got = [np.lib.stride_tricks.as_strided(out[o:], (oh, ow, 3), (dp, 3, 1)).copy() for o, dp, oh, ow in rects]
    return got, want, np.array_equal(out[keep], before[keep])


def test_paste_equals_the_host_yardstick_in_one_launch_and_alone(dev):
    from tatt_amd import io
    items = paste_items()
    got, want, outside = _run_paste(dev, items)                      # all items in one launch, one strip table
    for n, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (n, items[n][2:], int((g != w).sum()), g.size)
    assert outside
    painted = [(io.poly_owner_host(it[1], it[2], it[3]) >= 0).mean() for it in items]
    assert min(painted) < 0.5 and max(painted) == 1 and all(p > 0 for p in painted)        # the launches both paint and skip pixels
    assert {len(it[1].paste) for it in items} == {1, 2, 3, 4, 7}
    for n, it in enumerate(items):                                   # alone: the grid is sized by this item, its strips begin at row 0
        got, want, outside = _run_paste(dev, [it], seed=2 + n)
        assert np.array_equal(got[0], want[0]) and outside, (n, it[2:])


def test_paste_entry_refuses_and_a_stale_row_writes_nothing(dev):
    from tatt_amd import io, ops
    from tatt_amd.polys import poly_item_row, poly_strip_row
    lim = io.poly_limits()
    src = torch.randint(0, 256, (41 * 650 + 3 * 214,), dtype=torch.uint8, device=dev)   # to the last pixel's last byte
    dst = torch.full((16 + 80 * 612,), 7, dtype=torch.uint8, device=dev)
    maps = io.poly_matrices(ARC, 2)                                  # the (42, 214) line into the (80, 200) box
    table, start = [], 0
    for k, m in enumerate(maps.paste):
        table.append(poly_strip_row(2 * start, 2 * maps.widths[k], m, maps.seams[k - 1] if k else None, maps.seams[k] if k < 2 else None))
        start += maps.widths[k]

    def item(**kw):
        base = dict(src=0, hs=42, ws=214, sp=650, dst=16, oh=80, ow=200, dp=612, f=0, first=0, count=3)
        base.update({k: v for k, v in kw.items() if k in base})
        r = poly_item_row(*(base[k] for k in ("src", "hs", "ws", "sp", "dst", "oh", "ow", "dp", "f", "first", "count")))
        for i in range(11, 16):
            r[i] = kw.get("r%d" % i, 0)
        return r

    def run(r, dev_row=None, dev_table=None, db=None, n_strips=3):
        host, htab = torch.tensor([r], dtype=torch.int32), torch.tensor(table, dtype=torch.int32)
        d = torch.tensor([dev_row if dev_row is not None else r], dtype=torch.int32).to(dev)
        t = torch.tensor(dev_table if dev_table is not None else table, dtype=torch.int32).to(dev)
        P = lambda x: ctypes.c_void_p(x.data_ptr())
        return ops.LIB.tatt_poly_paste_u8(P(src), src.numel(), P(d), P(host), 1, P(t), P(htab), n_strips, P(dst),
                                          dst.numel() if db is None else db, ops.stream())
    assert run(item(r12=1)) == 1 and run(item(f=-1)) == 1
    assert run(item(oh=lim["side"] + 1)) == 2 and run(item(f=lim["feather"] + 1)) == 2 and run(item(count=0)) == 2
    assert run(item(src=1)) == 3 and run(item(dst=32)) == 3 and run(item(dp=599)) == 3 and run(item(), db=100) == 3
    assert run(item(first=1)) == 4 and run(item(), n_strips=2) == 4 and run(item(first=-1)) == 4
    bad_table = [list(r) for r in table]
    bad_table[2][1] = 0                                              # a strip without columns
    for stale in (item(r13=1), item(src=1), item(dst=32), item(dp=599), item(f=-2), item(ow=lim["side"] + 1), item(first=1),
                  item(count=lim["strips"] + 1)):
        assert run(item(), dev_row=stale) == 0
    assert run(item(), dev_table=bad_table) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7).all())
    assert run(item()) == 0
    torch.cuda.synchronize()
    assert bool((dst[:16] == 7).all()) and not bool((dst[16:] == 7).all())


# ---- the way in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (True, False), ids=("mask", "rgb"))
def test_poly_windows_equal_the_host_path(dev, mask):
    from tatt_amd import io, ops
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=mask, device=dev)
    scene = _img(1, HS, WS, 1)
    polys = [ONE, ARC, SCURVE, ARC8]
    want, lines = io.poly_windows_host(scene, polys, LR, 32, mask)
    calls, real = [], ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        got, got_lines, scene_dev = col.poly_windows(scene, polys, 32)
    finally:
        ops.call = real
    assert calls == ["tatt_warp_u8", "tatt_scene_windows"]           # ONE rectify launch for the 1 + 3 + 4 + 7 strips
    assert got_lines == lines and [len(ln.starts) for ln in lines] == [1, 2, 4, 3]
    assert got.shape == want.shape and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    assert scene_dev.shape == (HS, WS, 3) and scene_dev.dtype == torch.uint8 and np.array_equal(scene_dev.cpu().numpy(), np.asarray(scene))
    empty, none, scene_dev = col.poly_windows(scene, [], 32)
    assert empty.shape == (0, 3 + mask, 16, 64) and none == [] and np.array_equal(scene_dev.cpu().numpy(), np.asarray(scene))


def test_poly_windows_resize_a_crop_beyond_the_line_limits_on_the_device(dev):
    """windows of 32 x 256: a crop of 92 rows is more than the window kernel's intermediate holds (92 * 256 * 3 bytes), so ONE
    tatt_resize_u8 launch makes its (wl, 32) version on the device"""
    from tatt_amd import io, ops
    from tatt_amd.lines import _line_takes
    col = io.DeviceCollator(imgH=32, imgW=256, down_sample_scale=1, mask=True, device=dev)
    scene = _img(3, HS, WS, 1)
    big = ((10, 3), (100, 2), (190, 4), (188, 93), (100, 94), (12, 92))                       # N = 3
    polys = [ARC, big, ONE]
    bw, bh = io.poly_size(big)
    plan = io.poly_plan(scene, polys, (32, 256), 128, True)
    assert not _line_takes(bh, bw, 32, plan.lines[1].wl, 256, io.line_limits()) and len(plan.resize) == 1 and len(plan.arrays) == 1
    want, lines = io.poly_windows_host(scene, polys, (32, 256), 128, True)
    calls, real = [], ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        got, got_lines, _ = col.poly_windows(scene, polys, 128)
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
@pytest.mark.parametrize("polys", (DISJOINT, POLYS), ids=("disjoint", "layers"))
def test_scene_polys_export_equals_the_host_composition(dev, polys, feather):
    from tatt_amd import io, ops
    scene = _img(4, HS, WS, 0)
    col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=True, device=dev)
    ex = io.DeviceExporter(device=dev, rule="floor")
    _, lines, scene_dev = col.poly_windows(scene, polys, 32)
    n_layers = 1 + max(io.poly_layers(polys))
    assert n_layers == (1 if polys is DISJOINT else 2)
    sr = _sr_stack(lines, len(polys))
    calls, real = [], ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        pending = ex.scene_polys(scene_dev, sr.to(dev), lines, polys, 2, feather)
    finally:
        ops.call = real
    assert calls == ["tatt_line_blend", "tatt_resize_u8", "tatt_resize_u8"] + ["tatt_poly_paste_u8"] * n_layers
    got = pending.result()
    assert len(got) == 1 and got[0].size == (2 * WS, 2 * HS) and got[0].mode == "RGB"
    imgs = [io.blend_windows_host(sr[ln.first:ln.first + len(ln.starts)], ln.starts, ln.wl, 2, "floor") for ln in lines]
    _diff(got[0], io.poly_compose_host(scene, polys, imgs, 2, feather))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _generator(dev, cls="TSRN", seed=1234):
    import tatt_amd
    torch.manual_seed(seed)
    m = getattr(tatt_amd, cls)(**STD)
    m.load_state_dict(randomize_state_dict(m.state_dict()))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def tsrn_polys(dev):
    from tatt_amd.infer import SuperResolver
    up = SuperResolver(_generator(dev), batch_size=3, lr_size=LR, mask=True, rule="floor", keep_sr=True, stride=32)
    scene = _img(60, HS, WS, 1)
    pending = up.scene_polys(scene, POLYS, 3)
    return up, scene, pending, pending.result()


def _check_against_host(io, scene, polys, feather, pending, image):
    want_lr, lines = io.poly_windows_host(scene, polys, LR, 32, True)
    assert pending.lines == lines and pending.boxes == polys and pending.layers == io.poly_layers(polys)
    assert torch.equal(pending.lr.cpu(), want_lr)
    sr = pending.sr.cpu()
    assert sr.shape == (want_lr.shape[0], sr.shape[1], 32, 128)
    rows = iter(sr.split([len(ln.starts) for ln in lines]))
    assert image.mode == "RGB" and image.size == (2 * scene.size[0], 2 * scene.size[1])
    _diff(image, io.super_resolve_polys_host(scene, polys, lambda x: next(rows), LR, 32, True, "floor", feather=feather))


def test_super_resolver_scene_polys_equals_the_host_composition_of_its_own_sr(dev, tsrn_polys):
    from tatt_amd import io
    up, scene, pending, image = tsrn_polys
    assert pending.lr.shape[0] == 7 and sorted(up.sessions) == [1, 3]              # seven windows at batch_size 3: 3 + 3 + 1
    _check_against_host(io, scene, POLYS, 3, pending, image)
    assert not np.array_equal(np.asarray(image), np.asarray(scene.resize((2 * WS, 2 * HS), Image.BICUBIC)))


@pytest.mark.parametrize("feather", (0, 2))
def test_four_point_polygons_give_the_bytes_of_scene_quads(dev, tsrn_polys, feather):
    up, scene, _, _ = tsrn_polys
    quads = [ONE, THREE, PERSX]                                      # PERSX's bounding box meets THREE's
    a = up.scene_polys(scene, quads, feather)
    b = up.scene_quads(scene, quads, feather)
    assert torch.equal(a.lr, b.lr) and a.lines == b.lines and a.layers == b.layers == [0, 0, 1]
    _diff(a.result(), b.result())


def test_scene_polys_without_polygons_is_the_plain_upscale(dev, tsrn_polys):
    up, scene, _, _ = tsrn_polys
    n = len(up.sessions)
    p = up.scene_polys(scene, [])
    _diff(p.result(), scene.resize((2 * WS, 2 * HS), Image.BICUBIC))
    assert p.sr is None and p.lines == [] and p.boxes == [] and p.layers == [] and len(up.sessions) == n


def test_second_scene_polys_call_makes_no_host_wait_before_result(dev, tsrn_polys):
    from tatt_amd import io
    up, scene, pending, image = tsrn_polys
    again = _img(62, HS, WS, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = up.scene_polys(again, POLYS, 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check_against_host(io, again, POLYS, 0, p, p.result())
    _diff(up.scene_polys(scene, POLYS, 3).result(), image)           # and the first scene gives its bytes again


def test_scene_polys_with_a_reader(dev, tsrn_polys):
    """the picture byte for byte that without a reader; one reading per polygon, in input order: the reading of the host-blended line"""
    import tatt_amd
    from tatt_amd import io, read
    from tatt_amd.infer import SuperResolver
    up, scene, _, _ = tsrn_polys
    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    crnn.load_state_dict(randomize_state_dict(crnn.state_dict(), seed=11))
    crnn = crnn.to(dev).eval()
    rd = SuperResolver(up.gen, batch_size=4, lr_size=LR, mask=True, rule="floor", keep_sr=True, stride=32, reader=crnn)
    p = rd.scene_polys(scene, POLYS, 2)
    _diff(p.result(), up.scene_polys(scene, POLYS, 2).result())
    sr = p.sr.cpu()
    blended = [io.blend_windows_host(sr[ln.first:ln.first + len(ln.starts)], ln.starts, ln.wl, 2, "floor") for ln in p.lines]
    texts, readings = p.texts(), p.readings()
    assert len(texts) == len(POLYS) and texts == [r.text for r in readings]
    assert [r.rw for r in readings] == [io.read_width(ln.wl) for ln in p.lines]
    want = read.read_lines_host(blended, lambda x: rd.reader.forward(x.to(dev)).cpu(), scale=2, w=LR[1])
    for g, w in zip(readings, want):                                 # (another batch than the host's B = 1: strings and steps, not probabilities)
        assert g.text == w.text and g.chars == w.chars and g.steps == w.steps and g.rw == w.rw and g.squeezed == w.squeezed, (g, w)
    none = rd.scene_polys(scene, [])
    assert none.texts() == [] and none.readings() == []
    for decode in ("beam", "lexicon", "words"):                      # the other decodings take polygons as they take quads
        kw = dict(read_lexicon=["ab", "abc", "b"]) if decode != "beam" else {}
        other = SuperResolver(up.gen, batch_size=4, lr_size=LR, mask=True, rule="floor", stride=32, reader=crnn, read_decode=decode, **kw)
        q = other.scene_polys(scene, POLYS, 2)
        _diff(q.result(), p.result())
        assert len(q.readings()) == len(POLYS)


def test_scene_polys_refuses_a_recogniser_a_bad_stride_and_bad_polygons(dev, tsrn_polys):
    import tatt_amd
    from tatt_amd.infer import SuperResolver
    up, scene, _, _ = tsrn_polys
    rec = tatt_amd.CRNN(32, 1, 37, 256).to(dev).eval()
    with pytest.raises(ValueError, match="recogni"):
        SuperResolver(up.gen, recognizer=rec).scene_polys(scene, POLYS)
    with pytest.raises(ValueError, match="stride"):
        SuperResolver(up.gen, stride=16).scene_polys(scene, POLYS)
    for bad in (ARC[::-1], ARC[:7], (0, 0, 64, 16), ARC[:3] + ((201, 30),) + ARC[4:], ARC[:3] + ((110.0, 30),) + ARC[4:],
                ((20, 10), (21, 10), (60, 10), (60, 30), (21, 30), (20, 30))):
        with pytest.raises(ValueError, match="polygon 0"):
            up.scene_polys(scene, [bad])
    with pytest.raises(ValueError, match="feather"):
        up.scene_polys(scene, POLYS, -1)
