"""CPU: the host specification of the scene path (tatt_amd/scene.py): the box check, the window stack of all boxes, the paste layers, the
composition with its feather, the host halves of the launches, and the return codes of the C entries on host rows alone.  Everything
here is integer arithmetic on uint8 once Pillow has resized, so every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_ref as R

LR = (16, 64)
# over-wide (wl = 171, five windows) | touches two scene borders | plain | 4 x 4 | overlaps boxes 0 and 2
BOXES = [(5, 3, 155, 17), (0, 0, 64, 16), (100, 30, 160, 48), (7, 9, 11, 13), (60, 10, 120, 40)]


def _img(seed, hs, ws, kind=1):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, kind), "RGB")


def _line_images(seed, boxes, scale=2, lr=LR, stride=32):
    """a random uint8 'SR line' per box, of the size the blend gives: (scale * wl, scale * h)"""
    from tatt_amd import io
    rng = np.random.default_rng(seed)
    out = []
    for x0, y0, x1, y1 in boxes:
        wl = io.line_plan((x1 - x0, y1 - y0), lr, stride)[0]
        out.append(rng.integers(0, 256, (scale * lr[0], scale * wl, 3), dtype=np.uint8))
    return out


# ---- layers -------------------------------------------------------------------------------------------------------------------------
def test_scene_layers_example_and_disjointness():
    from tatt_amd import io
    assert io.scene_layers(BOXES) == [0, 1, 0, 2, 2]
    assert io.scene_layers([]) == [] and io.scene_layers([(0, 0, 4, 4), (4, 0, 8, 4)]) == [0, 0]        # touching sides do not intersect
    rng = np.random.default_rng(0)
    boxes = [(int(x), int(y), int(x) + int(w), int(y) + int(h)) for x, y, w, h in
             zip(rng.integers(0, 90, 40), rng.integers(0, 40, 40), rng.integers(4, 30, 40), rng.integers(4, 20, 40))]
    layers = io.scene_layers(boxes)
    hit = lambda a, b: a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]
    for i in range(40):
        for j in range(i):
            if hit(boxes[i], boxes[j]):
                assert layers[i] > layers[j]


@pytest.mark.parametrize("feather", (0, 3))
def test_layer_by_layer_equals_box_by_box(feather):
    from tatt_amd import io
    scene = _img(1, 48, 160, 0)
    imgs = _line_images(2, BOXES)
    layers = io.scene_layers(BOXES)
    order = sorted(range(len(BOXES)), key=lambda k: (layers[k], k))
    assert order != list(range(len(BOXES)))
    a = io.scene_compose_host(scene, BOXES, imgs, 2, feather)
    b = io.scene_compose_host(scene, BOXES, imgs, 2, feather, order=order)
    assert np.array_equal(np.asarray(a), np.asarray(b))
    plan = io.paste_plan(scene.size, BOXES, *_blend(BOXES)[:2], 2, 32, feather)
    assert plan.order == order and plan.layers == layers and plan.counts == [2, 1, 2]


# ---- windows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (True, False))
def test_scene_windows_are_the_line_windows_of_each_crop(mask):
    from tatt_amd import io
    scene = _img(3, 48, 160)
    stack, lines = io.scene_windows_host(scene, BOXES, LR, 32, mask)
    want = [io.line_windows_host(scene.crop(b), LR, 32, mask) for b in BOXES]
    assert torch.equal(stack, torch.cat(want)) and stack.shape == (9, 3 + mask, 16, 64)
    assert lines[0] == io.Line(171, [0, 32, 64, 96, 107], 0)
    assert [(ln.wl, ln.starts, ln.first) for ln in lines[1:]] == [(64, [0], 5), (64, [0], 6), (64, [0], 7), (64, [0], 8)]
    empty, none = io.scene_windows_host(scene, [], LR, 32, mask)
    assert empty.shape == (0, 3 + mask, 16, 64) and none == []


def test_crop_then_resize_is_the_restated_resampler_on_the_box_alone():
    scene = _img(4, 48, 160)
    a = np.asarray(scene)
    for x0, y0, x1, y1 in BOXES:
        want = np.asarray(scene.crop((x0, y0, x1, y1)).resize((64, 16), Image.BICUBIC))
        assert np.array_equal(R.resize_bicubic(a[y0:y1, x0:x1], (64, 16)), want)


# ---- the composition ----------------------------------------------------------------------------------------------------------------
def test_compose_without_feather_is_image_paste():
    from tatt_amd import io
    scene = _img(5, 48, 160, 0)
    imgs = _line_images(6, BOXES, 2)
    want = scene.resize((320, 96), Image.BICUBIC)
    for (x0, y0, x1, y1), im in zip(BOXES, imgs):
        want.paste(Image.fromarray(im, "RGB").resize((2 * (x1 - x0), 2 * (y1 - y0)), Image.BICUBIC), (2 * x0, 2 * y0))
    got = io.scene_compose_host(scene, BOXES, imgs, 2)
    assert got.size == (320, 96) and got.mode == "RGB" and np.array_equal(np.asarray(got), np.asarray(want))
    assert np.array_equal(np.asarray(io.scene_compose_host(scene, [], [], 2)), np.asarray(scene.resize((320, 96), Image.BICUBIC)))
    assert np.array_equal(np.asarray(io.scene_compose_host(scene, [], [], 1)), np.asarray(scene))


def test_feather_two_by_hand():
    """one 8 x 6 box at scale 1 in a constant scene of 100, a constant line of 10, F = 2, D = 3: ring 0 takes a = 1:
    (2 * (10 + 2 * 100) + 3) // 6 = 70, ring 1 a = 2: (2 * (20 + 100) + 3) // 6 = 40, the inside a = 3: 10"""
    from tatt_amd import io
    scene = Image.fromarray(np.full((12, 20, 3), 100, np.uint8), "RGB")
    line = np.full((16, 64, 3), 10, np.uint8)
    got = np.asarray(io.scene_compose_host(scene, [(3, 2, 11, 8)], [line], 1, 2))
    want = np.full((12, 20), 100)
    want[2:8, 3:11] = 70
    want[3:7, 4:10] = 40
    want[4:6, 5:9] = 10
    assert np.array_equal(got, np.repeat(want[:, :, None], 3, 2).astype(np.uint8))
    # rounding half up: old 101, new 10, a = 1 of 2: (2 * (10 + 101) + 2) // 4 = 56 (55.5 rounds up)
    scene = Image.fromarray(np.full((12, 20, 3), 101, np.uint8), "RGB")
    got = np.asarray(io.scene_compose_host(scene, [(3, 2, 11, 8)], [line], 1, 1))
    assert got[2, 3, 0] == 56 and got[3, 4, 0] == 10 and got[1, 3, 0] == 101
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError):
            io.scene_compose_host(scene, [(3, 2, 11, 8)], [line], 1, bad)


def test_host_composition_with_a_model_as_a_callable():
    from tatt_amd import io
    up = lambda x: x[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3)
    scene = _img(7, 48, 160, 0)
    got = io.super_resolve_scene_host(scene, BOXES, up, LR, 32, True, "floor", feather=1)
    stack, lines = io.scene_windows_host(scene, BOXES, LR, 32, True)
    imgs = [io.blend_windows_host(up(stack[ln.first:ln.first + len(ln.starts)]), ln.starts, ln.wl, 2) for ln in lines]
    assert np.array_equal(np.asarray(got), np.asarray(io.scene_compose_host(scene, BOXES, imgs, 2, 1)))
    plain = io.super_resolve_scene_host(scene, [], up, LR, scale=2)
    assert np.array_equal(np.asarray(plain), np.asarray(scene.resize((320, 96), Image.BICUBIC)))
    with pytest.raises(ValueError):
        io.super_resolve_scene_host(scene, [], up, LR)
    with pytest.raises(ValueError):
        io.super_resolve_scene_host(scene, BOXES, up, LR, scale=4)


# ---- scene_check --------------------------------------------------------------------------------------------------------------------
def test_scene_check_refuses():
    from tatt_amd import io
    size = (160, 48)
    assert io.SCENE_MIN_SIDE == 4
    assert io.scene_check(size, BOXES) == BOXES
    assert io.scene_check(size, [np.array([0, 0, 160, 48])]) == [(0, 0, 160, 48)]
    for bad in ((0, 0, 3, 16), (0, 0, 16, 3), (100, 0, 161, 16), (0, 40, 16, 49), (8, 0, 8, 16), (9, 0, 8, 16), (-1, 0, 8, 16),
                (0.0, 0, 8, 16), (0, 0, 8.5, 16), (0, 0, 8), "abcd", None):
        with pytest.raises(ValueError, match="box 1"):
            io.scene_check(size, [BOXES[0], bad])
    lim = io.scene_limits()
    io.scene_check(size, [BOXES[1]] * lim["boxes"])
    with pytest.raises(ValueError, match="boxes"):
        io.scene_check(size, [BOXES[1]] * (lim["boxes"] + 1))


# ---- plans --------------------------------------------------------------------------------------------------------------------------
def _blend(boxes, scale=2, H=32, W=128):
    from tatt_amd import io
    lines, first = [], 0
    for x0, y0, x1, y1 in boxes:
        wl, starts = io.line_plan((x1 - x0, y1 - y0), LR, 32)
        lines.append(io.Line(wl, starts, first))
        first += len(starts)
    desc, starts, nbytes = io.blend_plan(lines, first, H, W, scale)
    return desc, nbytes, lines


def test_scene_plan_rows_offsets_and_the_host_resize_fallback():
    from tatt_amd import io
    lim = io.line_limits()
    Hs, Ws = lim["rows"] + 60, 300
    scene = _img(8, Hs, Ws, 0)
    tall = (10, 5, 290, lim["rows"] + 45)                              # more rows than the window kernel resamples: PIL on the host
    boxes = [(5, 3, 155, 17), tall, (0, 0, 64, 16)]
    plan = io.scene_plan(scene, boxes, LR, 32, True, lim)
    assert len(plan.arrays) == 2 and plan.offsets[0] == 0 and np.array_equal(plan.arrays[0], np.asarray(scene))
    wl = io.line_plan((280, lim["rows"] + 40), LR, 32)[0]
    assert plan.arrays[1].shape == (16, wl, 3)
    assert np.array_equal(plan.arrays[1], np.asarray(scene.crop(tall).resize((wl, 16), Image.BICUBIC)))
    assert all(o % 16 == 0 for o in plan.offsets) and plan.offsets[1] >= Hs * Ws * 3 and plan.nbytes >= plan.offsets[1] + 16 * wl * 3
    d = plan.desc
    assert d.dtype == np.int32 and d.shape == (5 + 1 + 1, 16) and not d[:, 12:].any()
    assert d[:5, :12].tolist() == [[0, 14, 150, 16, 171, x, 64, 1, k * 4096, 900, 5, 3] for k, x in enumerate((0, 32, 64, 96, 107))]
    assert d[5, :12].tolist() == [plan.offsets[1], 16, wl, 16, wl, 0, 64, 1, 5 * 4096, 3 * wl, 0, 0]
    assert d[6, :12].tolist() == [0, 16, 64, 16, 64, 0, 64, 1, 6 * 4096, 900, 0, 0]
    assert [ln.first for ln in plan.lines] == [0, 5, 6] and plan.out_floats == 7 * 4096
    flat = np.zeros(io.scene_fill(None, plan)[1], np.uint8)
    pix, used = io.scene_fill(flat, plan)
    assert pix % 16 == 0 and pix >= d.nbytes and used == flat.size
    assert np.array_equal(flat[:d.nbytes].view(np.int32), d.reshape(-1))
    for a, o in zip(plan.arrays, plan.offsets):
        assert np.array_equal(flat[pix + o:pix + o + a.size], a.reshape(-1))
    # the same windows either way: cutting the host-resized line is what the host path does
    want = io.line_windows_host(scene.crop(tall), LR, 32, True)
    line = Image.fromarray(plan.arrays[1], "RGB")
    assert torch.equal(torch.stack([io.resize_normalize(line.crop((0, 0, 64, 16)), (64, 16), True)]), want)
    with pytest.raises(ValueError):
        io.scene_plan(scene.convert("L"), boxes, LR, 32, True, lim)
    none = io.scene_plan(scene, [], LR, 32, True, lim)
    assert none.desc.shape == (0, 16) and none.out_floats == 0 and none.nbytes >= Hs * Ws * 3


def test_paste_plan_rows():
    from tatt_amd import io
    desc, nbytes, lines = _blend(BOXES)
    plan = io.paste_plan((160, 48), BOXES, desc, nbytes, 2, 32, 3)
    assert plan.canvas_off % 16 == 0 and plan.canvas_off >= nbytes and plan.pitch == 960
    assert plan.nbytes == plan.canvas_off + 96 * 960
    assert plan.rows.dtype == np.int32 and plan.rows.shape == (6, 16) and not plan.rows[:, 9:].any()
    assert plan.rows[0, :9].tolist() == [0, 48, 160, 480, plan.canvas_off, 96, 320, 960, 0]
    for r, k in enumerate(plan.order):
        x0, y0, x1, y1 = BOXES[k]
        assert plan.rows[1 + r, :9].tolist() == [int(desc[k, 6]), 32, 2 * lines[k].wl, int(desc[k, 7]),
                                                plan.canvas_off + 2 * y0 * 960 + 6 * x0, 2 * (y1 - y0), 2 * (x1 - x0), 960, 3]
    assert all(int(v) % 16 == 0 for v in desc[:, 6])
    empty = io.paste_plan((160, 48), [], desc[:0], 0, 2, 0)
    assert empty.rows.shape == (1, 16) and empty.canvas_off == 0 and empty.counts == [] and empty.nbytes == 96 * 960
    with pytest.raises(ValueError):
        io.paste_plan((160, 48), BOXES, desc[:4], nbytes, 2, 32)
    with pytest.raises(ValueError):
        io.paste_plan((160, 48), BOXES, desc, nbytes, 2, 32, -1)
    with pytest.raises(ValueError):
        io.paste_plan((160, 48), BOXES, desc, nbytes, 2, 32, io.scene_limits()["feather"] + 1)


def test_plans_refuse_what_does_not_fit_32_bit_offsets():
    from tatt_amd import io
    lim = io.scene_limits()
    with pytest.raises(ValueError, match="32-bit"):                    # 16384 x 16384 x 3 x 4 bytes of canvas
        io.paste_plan((16384, 16384), [], np.zeros((0, 8), np.int32), 0, 2, 0, limits=lim)
    with pytest.raises(ValueError, match="side"):
        io.paste_plan((lim["side"], 8), [], np.zeros((0, 8), np.int32), 0, 2, 0, limits=lim)

    a = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (32768, 32768, 3), (0, 0, 0))    # (3 GiB of scene, not allocated)
    img = type("S", (), {"mode": "RGB", "size": (32768, 32768), "__array__": lambda self, *k, **kw: a})()
    with pytest.raises(ValueError, match="32-bit"):
        io.scene_plan(img, [], LR, 32, True)


# ---- the C entries on host rows alone -----------------------------------------------------------------------------------------------
def test_scene_limits_need_no_gpu():
    from tatt_amd import io
    lim = io.scene_limits()
    assert set(lim) == {"side", "boxes", "tile_h", "tile_w", "down", "feather", "inter_rows", "items"}
    assert lim["tile_h"] >= 8 and lim["tile_w"] >= 8 and lim["down"] >= 16 and lim["side"] >= 8192 and lim["boxes"] >= 256
    assert lim["feather"] >= 16 and lim["items"] >= lim["boxes"] and lim["inter_rows"] >= 4 * lim["down"] + 2


def _rc(name, rows, *sizes):
    """the entry's return code for host rows it must refuse before it touches a device (the device pointers are never read)"""
    from tatt_amd import ops
    host = np.ascontiguousarray(np.array(rows, np.int32))
    dummy = ctypes.c_void_p(host.ctypes.data)
    if name == "tatt_scene_windows":
        return ops.LIB.tatt_scene_windows(dummy, sizes[0], dummy, dummy, len(rows), dummy, sizes[1], None)
    return ops.LIB.tatt_resize_u8(dummy, sizes[0], dummy, dummy, len(rows), dummy, sizes[1], None)


def test_window_entry_return_codes_on_host_rows():
    from tatt_amd import io
    lim = io.line_limits()
    nb, nf = 48 * 160 * 3, 4 * 16 * 64
    row = lambda **kw: [kw.get(k, v) for k, v in (("src", 0), ("hs", 14), ("ws", 150), ("h", 16), ("wl", 171), ("x0", 0), ("w", 64),
                                                  ("mask", 1), ("out", 0), ("pitch", 480), ("bx", 5), ("by", 3), ("r12", 0), ("r13", 0),
                                                  ("r14", 0), ("r15", 0))]
    run = lambda r, nbytes=nb, floats=nf: _rc("tatt_scene_windows", [r], nbytes, floats)
    assert run(row(r12=1)) == 1 and run(row(r15=-1)) == 1
    assert _rc("tatt_scene_windows", [], nb, nf) == 1 and run(row(), nbytes=0) == 1
    assert run(row(x0=108)) == 2 and run(row(x0=-1)) == 2 and run(row(wl=63)) == 2 and run(row(hs=0)) == 2
    assert run(row(h=lim["h"] + 1)) == 2 and run(row(w=lim["w"] + 1)) == 2 and run(row(wl=lim["wl"] + 1)) == 2
    assert run(row(hs=lim["rows"] + 1)) == 2 and run(row(ws=lim["cols"] + 1, pitch=3 * (lim["cols"] + 6))) == 2
    assert run(row(bx=11)) == 3 and run(row(bx=-1)) == 3 and run(row(by=-1)) == 3 and run(row(src=-16)) == 3
    assert run(row(by=35)) == 3 and run(row(pitch=464)) == 3 and run(row(), nbytes=16 * 480 + 465 - 1) == 3
    assert run(row(out=1)) == 3 and run(row(out=-1)) == 3 and run(row(mask=0), floats=3 * 1024 - 1) == 3


def test_resize_entry_return_codes_on_host_rows():
    from tatt_amd import io
    lim = io.scene_limits()
    sb, db = 70 * 450, 16 + 140 * 912
    row = lambda **kw: [kw.get(k, v) for k, v in (("src", 0), ("hs", 70), ("ws", 150), ("sp", 450), ("dst", 16), ("oh", 140), ("ow", 300),
                                                  ("dp", 912), ("f", 0))] + [kw.get("r%d" % i, 0) for i in range(9, 16)]
    run = lambda r, s=sb, d=db: _rc("tatt_resize_u8", [r], s, d)
    assert run(row(r9=1)) == 1 and run(row(r15=7)) == 1 and run(row(f=-1)) == 1
    assert _rc("tatt_resize_u8", [], sb, db) == 1 and run(row(), d=0) == 1
    assert run(row(hs=0)) == 2 and run(row(ow=0)) == 2 and run(row(f=lim["feather"] + 1)) == 2
    assert run(row(oh=4, dp=912)) == 2 and run(row(ow=9)) == 2          # 70 rows -> 4, 150 columns -> 9: beyond 16 : 1
    assert run(row(oh=lim["side"] + 1)) == 2 and run(row(ws=lim["side"] + 1)) == 2
    assert _rc("tatt_resize_u8", [row()] * (lim["items"] + 1), sb, db) == 2
    assert run(row(src=-1)) == 3 and run(row(sp=449)) == 3 and run(row(), s=sb - 1) == 3 and run(row(src=1)) == 3
    assert run(row(dst=-16)) == 3 and run(row(dp=899)) == 3 and run(row(), d=db - 13) == 3 and run(row(dst=32)) == 3


# ---- build --------------------------------------------------------------------------------------------------------------------------
def test_scene_source_is_built_without_contraction():
    from tatt_amd import build
    assert "scene.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["scene.hip"]
    assert build.SOURCES.index("lines.hip") < build.SOURCES.index("scene.hip")


def test_super_resolver_has_no_cpu_path_for_scenes():
    import tatt_amd
    from tatt_amd.infer import SuperResolver
    assert hasattr(SuperResolver, "scene")
    m = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32)
    with pytest.raises(RuntimeError, match="GPU"):
        SuperResolver(m)
