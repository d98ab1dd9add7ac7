"""CPU: the host specification of quadrilateral text boxes (tatt_amd/quads.py): the quad check, the rectified size, the integer matrices
against an independent derivation (tests/quad_warp_ref.py), the warp against a scalar restatement, what axis-aligned quads must give
(the bytes of the box path), a round trip, the host halves of the launches and the return codes of the C entry on host rows alone.
Everything but the round trip is exact integer arithmetic: np.array_equal / ==, no tolerance."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_ref as R
from tests import quad_warp_ref as Q0

LR = (16, 64)
SIZE = (211, 97)                                                     # (Ws, Hs) of the scenes here
AXIS = ((20, 10), (120, 10), (120, 40), (20, 40))
ROT15 = ((30, 20), (150, 50), (142, 80), (22, 50))                   # about 14 degrees
ROT90 = ((60, 10), (60, 90), (40, 90), (40, 10))                     # vertical text, read downwards
PERSX = ((30, 10), (180, 25), (175, 70), (35, 90))                   # the left side 80 high, the right one 45
PERSXY = ((40, 15), (170, 8), (190, 85), (25, 60))                   # no two sides parallel
FIVE = [AXIS, ROT15, ROT90, PERSX, PERSXY]


def _img(seed, hs, ws, kind=1):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, kind), "RGB")


def _smooth(seed):
    """a smooth scene: random 13 x 27 up-scaled bicubically to 97 x 211.  The random values span 64 .. 191 so that the bicubic overshoot
    never clips at 0 or 255 (a clipped plateau has a kink, and a kink is not smooth)."""
    small = np.random.default_rng(seed).integers(64, 192, (13, 27, 3), dtype=np.uint8)
    return Image.fromarray(small, "RGB").resize(SIZE, Image.BICUBIC)


# ---- the check and the size ---------------------------------------------------------------------------------------------------------
def test_quad_check_refuses_and_accepts():
    from tatt_amd import io
    ok = io.quad_check(SIZE, FIVE)
    assert ok == [tuple(tuple(p) for p in q) for q in FIVE]
    assert io.quad_check(SIZE, [((0, 0), (211, 0), (211, 97), (0, 97))]) == [((0, 0), (211, 0), (211, 97), (0, 97))]   # touches the border
    assert io.quad_check(SIZE, [[[20, 10], [120, 10], [120, 40], [20, 40]]]) == [AXIS] and io.quad_check(SIZE, []) == []
    bad = [((20, 10), (120, 10), (120, 40)),                         # three points
           (20, 10, 120, 40),                                        # a box
           ((20, 10), (120, 10), (120, 40), (20, 40.0)),             # a float
           ((20, 10), (120, 10), (120, 40), (20, True)),             # a bool
           ((20, 10), (212, 10), (212, 40), (20, 40)),               # leaves the image
           ((20, -1), (120, 10), (120, 40), (20, 40)),
           ((20, 10), (20, 40), (120, 40), (120, 10)),               # counter-clockwise
           ((20, 10), (120, 10), (70, 20), (20, 40)),                # not convex
           ((20, 10), (70, 10), (120, 10), (20, 40)),                # three points on a line
           ((20, 10), (120, 10), (120, 13), (20, 13)),               # 3 high
           ((20, 10), (23, 10), (23, 40), (20, 40)),                 # 3 wide
           ((20, 10), (120, 10), (120, 30), (20, 51))]               # the left side 41, the right one 20: beyond 2 : 1
    for q in bad:
        with pytest.raises(ValueError, match="quad 1"):
            io.quad_check(SIZE, [AXIS, q])
    assert io.quad_check(SIZE, [((20, 10), (120, 10), (120, 30), (20, 50))])               # exactly 2 : 1 is taken
    with pytest.raises(ValueError, match="at most"):
        io.quad_check(SIZE, [AXIS, ROT15], dict(io.scene_limits(), boxes=1))
    with pytest.raises(ValueError, match="image"):
        io.quad_check((0, 97), [])


def test_quad_size_on_hand_computed_quads():
    from tatt_amd import io
    assert io.quad_size(AXIS) == (100, 30)
    assert io.quad_size(((10, 0), (40, 40), (32, 46), (2, 6))) == (50, 10)                 # a 3-4-5 side: (30, 40) and (-8, 6)
    assert io.quad_size(((4, 0), (11, 7), (7, 11), (0, 4))) == (10, 6)                     # sqrt(98) = 9.90 -> 10, sqrt(32) = 5.66 -> 6
    assert io.quad_size(PERSX) == (151, 80)                          # the longer of (150, 15) and (140, -20); of (5, 80) and (-5, 45)
    assert io.quad_size(ROT90) == (80, 20)
    assert io.quad_bbox(PERSXY) == (25, 8, 190, 85)
    for q in FIVE:
        assert io.quad_size(q) == Q0.size(q)


# ---- the matrices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1, 2))
@pytest.mark.parametrize("k", range(5), ids=("axis", "rot15", "rot90", "persx", "persxy"))
def test_matrices_equal_the_independent_derivation(k, scale):
    from tatt_amd import io
    quad = FIVE[k]
    m_r, m_p, bbox = io.quad_matrices(quad, scale)
    w_r, w_p, w_box = Q0.matrices(quad, scale)
    assert tuple(m_r) == w_r and tuple(m_p) == w_p and bbox == w_box
    assert all(isinstance(v, int) for v in m_r + m_p)
    bw, bh = io.quad_size(quad)
    for (u, v), (x, y) in zip(((0, 0), (bw, 0), (bw, bh), (0, bh)), quad):               # rectangle corners -> quad corners
        X, Y, Wd = (m_r[3 * r] * 2 * u + m_r[3 * r + 1] * 2 * v + m_r[3 * r + 2] for r in range(3))
        assert Wd > 0 and abs(Fraction(X, Wd) - x) <= Fraction(1, 2 ** 16) and abs(Fraction(Y, Wd) - y) <= Fraction(1, 2 ** 16)
    s = scale
    for (u, v), (x, y) in zip(((0, 0), (bw, 0), (bw, bh), (0, bh)), quad):               # and back: quad corners -> the line's corners
        J, I = 2 * s * (x - bbox[0]), 2 * s * (y - bbox[1])
        X, Y, Wd = (m_p[3 * r] * J + m_p[3 * r + 1] * I + m_p[3 * r + 2] for r in range(3))
        assert Wd > 0 and abs(Fraction(X, Wd) - s * u) <= Fraction(1, 2 ** 16) and abs(Fraction(Y, Wd) - s * v) <= Fraction(1, 2 ** 16)


def test_axis_aligned_matrices_are_the_crop_and_the_paste():
    from tatt_amd import io
    one = 1 << io.QUAD_SHIFT
    m_r, m_p, bbox = io.quad_matrices(AXIS, 2)
    assert m_r == (one // 2, 0, 20 * one, 0, one // 2, 10 * one, 0, 0, one) and m_p == (one // 2, 0, 0, 0, one // 2, 0, 0, 0, one)
    assert bbox == (20, 10, 120, 40)


def test_plan_checks_raise_for_a_constructed_overflow():
    from tatt_amd import quads
    F = Fraction
    eye = lambda a=1, g=0, c=1: [[F(a), F(0), F(0)], [F(0), F(1), F(0)], [F(g), F(0), F(c)]]
    assert quads._integer(eye(), 1, 1, 8, 8, True, "t") == (1 << 36, 0, 0, 0, 1 << 36, 0, 0, 0, 1 << 36)
    with pytest.raises(ValueError, match="62 bits"):
        quads._integer(eye(2 ** 30), 1, 1, 8, 8, True, "t")          # an entry of 66 bits
    with pytest.raises(ValueError, match="62 bits"):
        quads._integer(eye(2 ** 10), 1, 1, 8, 32768, True, "t")      # 256 X = 2^8 2^46 65535 at the right-hand corner pixels
    quads._integer(eye(2 ** 10), 1, 1, 8, 64, True, "t")
    with pytest.raises(ValueError, match="horizon"):
        quads._integer(eye(1, -1, 50), 1, 1, 8, 100, True, "t")      # Wd = 50 - J turns negative inside the rectangle
    quads._integer(eye(1, -1, 50), 1, 1, 8, 100, False, "t")         # a paste only skips such pixels
    with pytest.raises(ValueError, match="singular"):
        quads._integer(eye(1, -1, 50), 50, 1, 8, 100, False, "t")


# ---- the warp -----------------------------------------------------------------------------------------------------------------------
def test_warp_equals_the_scalar_restatement_in_both_modes():
    from tatt_amd import io
    src = R.make_image(np.random.default_rng(5), 40, 90, 1)
    quad = ((8, 5), (80, 12), (76, 36), (10, 30))
    io.quad_check((90, 40), [quad])
    bw, bh = io.quad_size(quad)
    m_r, m_p, (x0, y0, x1, y1) = io.quad_matrices(quad, 1)
    crop = io.warp_u8_host(src, m_r, bh, bw)
    assert crop.shape == (bh, bw, 3) and crop.dtype == np.uint8
    assert np.array_equal(crop, np.array(Q0.warp(src, m_r, bh, bw), np.uint8))
    wide = io.warp_u8_host(src, m_r, bh + 30, bw + 30)               # beyond the rectangle: taps clamped to the border
    assert np.array_equal(wide, np.array(Q0.warp(src, m_r, bh + 30, bw + 30), np.uint8)) and np.array_equal(wide[:bh, :bw], crop)
    old = np.random.default_rng(6).integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    for feather in (0, 3):
        want = np.array(Q0.warp(crop, m_p, y1 - y0, x1 - x0, old, feather), np.uint8)
        dst = old.copy()
        got = io.warp_u8_host(crop, m_p, y1 - y0, x1 - x0, dst, feather)
        assert got is dst and np.array_equal(got, want), feather
        inside = io.warp_inside_host(m_p, y1 - y0, x1 - x0, bh, bw)
        assert np.array_equal(got[~inside], old[~inside]) and 0.5 < inside.mean() < 1
    # a matrix whose horizon crosses the destination: outside pixels are zero in mode 0 and kept in mode 1
    m = (1 << 36, 0, 0, 0, 1 << 36, 0, -(1 << 36), 0, 40 << 36)
    z = io.warp_u8_host(src, m, 12, 30)
    assert np.array_equal(z, np.array(Q0.warp(src, m, 12, 30), np.uint8)) and not z[:, 20:].any() and z[:, :19].any()
    keep = old[:12, :30].copy()
    assert np.array_equal(io.warp_u8_host(src, m, 12, 30, keep.copy(), 2), np.array(Q0.warp(src, m, 12, 30, keep, 2), np.uint8))


def test_axis_aligned_rectify_is_the_crop():
    from tatt_amd import io
    scene = _img(7, 97, 211)
    for quad, box in ((AXIS, (20, 10, 120, 40)), (((0, 0), (211, 0), (211, 97), (0, 97)), (0, 0, 211, 97))):
        assert np.array_equal(io.quad_rectify_host(scene, quad), np.asarray(scene.crop(box)))


def _fake_model(x):
    """a deterministic stand-in for a generator: (n, 4, h, w) -> (n, 4, 2 h, 2 w), values below 0 and above 1 included"""
    up = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return up * 1.3 - 0.15 + 0.05 * torch.arange(up.shape[-1]).remainder(3)


@pytest.mark.parametrize("feather", (0, 3))
def test_axis_aligned_quads_give_the_bytes_of_the_box_path(feather):
    from tatt_amd import io
    scene = _img(8, 97, 211)
    boxes = [(20, 10, 170, 40), (100, 30, 200, 70), (5, 50, 25, 60)]                       # the first two overlap
    quads = [((x0, y0), (x1, y0), (x1, y1), (x0, y1)) for x0, y0, x1, y1 in boxes]
    want_stack, want_lines = io.scene_windows_host(scene, boxes, LR, 32, True)
    stack, lines = io.quad_windows_host(scene, quads, LR, 32, True)
    assert lines == want_lines and torch.equal(stack, want_stack)
    a = io.super_resolve_quads_host(scene, quads, _fake_model, LR, 32, True, "floor", feather=feather)
    b = io.super_resolve_scene_host(scene, boxes, _fake_model, LR, 32, True, "floor", feather=feather)
    assert a.size == (422, 194) and np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(np.asarray(io.super_resolve_quads_host(scene, [], _fake_model, scale=2)),
                          np.asarray(scene.resize((422, 194), Image.BICUBIC)))


@pytest.mark.parametrize("quad", (ROT15, PERSX), ids=("rotated", "perspective"))
def test_round_trip_returns_the_scene_inside_the_quad_and_touches_nothing_outside(quad):
    """rectify, paste back at scale 1: two bilinear samplings of a smooth scene.  Bound (set with the feature): the mean absolute
    difference inside the quad is at most 1.0 grey level; a transposed or inverted matrix costs tens of levels."""
    from tatt_amd import io
    scene = _smooth(11)
    a = np.asarray(scene)
    crop = io.quad_rectify_host(scene, quad)
    out = np.asarray(io.quad_compose_host(scene, [quad], [crop], 1, 0))
    bw, bh = io.quad_size(quad)
    _, m_p, (x0, y0, x1, y1) = io.quad_matrices(quad, 1)
    inside = np.zeros(a.shape[:2], bool)
    inside[y0:y1, x0:x1] = io.warp_inside_host(m_p, y1 - y0, x1 - x0, bh, bw)
    mad = float(np.abs(out.astype(int) - a.astype(int))[inside].mean())
    print("round trip: mean |diff| inside = %.4f" % mad)
    assert mad <= 1.0, mad
    assert np.array_equal(out[~inside], a[~inside])
    area = abs(sum(quad[i][0] * quad[(i + 1) % 4][1] - quad[(i + 1) % 4][0] * quad[i][1] for i in range(4))) / 2
    share = inside[y0:y1, x0:x1].mean()
    assert abs(share - area / ((x1 - x0) * (y1 - y0))) <= 0.02, (share, area)
    swapped = np.asarray(io.quad_compose_host(scene, [quad], [crop[::-1, ::-1]], 1, 0))   # (what the bound is there to catch)
    assert float(np.abs(swapped.astype(int) - a.astype(int))[inside].mean()) > 10


def test_layer_by_layer_equals_quad_by_quad():
    from tatt_amd import io
    scene = _img(9, 97, 211)
    quads = [ROT15, PERSXY, ROT90, AXIS]
    layers = io.quad_layers(quads)
    assert layers == [0, 1, 2, 3] or max(layers) >= 1
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (32, 2 * io.line_plan(io.quad_size(q), LR, 32)[0], 3), dtype=np.uint8) for q in quads]
    order = sorted(range(len(quads)), key=lambda k: (layers[k], k))
    for feather in (0, 2):
        a = io.quad_compose_host(scene, quads, imgs, 2, feather)
        b = io.quad_compose_host(scene, quads, imgs, 2, feather, order=order)
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- the host halves of the launches ------------------------------------------------------------------------------------------------
def _words(row, k):
    lo, hi = int(row[10 + 2 * k]) & 0xFFFFFFFF, int(row[11 + 2 * k])
    return (hi << 32) | lo


def test_quad_plan_rows_and_offsets():
    from tatt_amd import io
    from tatt_amd.quads import QUAD_DESC
    scene = _img(10, 97, 211)
    quads = [AXIS, PERSX, ((5, 50), (25, 50), (25, 60), (5, 60))]
    plan = io.quad_plan(scene, quads, LR, 32, True)
    stack, lines = io.quad_windows_host(scene, quads, LR, 32, True)
    assert plan.lines == lines and plan.quads == quads and len(plan.desc) == stack.shape[0] and plan.out_floats == stack.numel()
    assert plan.warp.shape == (3, QUAD_DESC) and plan.resize.shape == (0, 16) and len(plan.arrays) == 1
    assert plan.upload == -(-97 * 211 * 3 // 16) * 16
    end = plan.upload
    for k, (q, row) in enumerate(zip(quads, plan.warp)):
        bw, bh = io.quad_size(q)
        assert list(row[:10]) == [0, 97, 211, 633, end, bh, bw, 3 * bw, 0, 0] and row[4] % 16 == 0 and not row[28:].any()
        assert tuple(_words(row, i) for i in range(9)) == io.quad_matrices(q, 1)[0]
        for d in plan.desc[lines[k].first:lines[k].first + len(lines[k].starts)]:
            assert list(d[:5]) == [row[4], bh, bw, 16, lines[k].wl] and list(d[9:]) == [3 * bw, 0, 0, 0, 0, 0, 0]
        end += -(-bh * bw * 3 // 16) * 16
    assert plan.nbytes == end
    o_warp, o_resize, o_desc, pix, used, total = io.quad_fill(None, plan)
    assert (o_warp, o_resize) == (0, 3 * QUAD_DESC * 4) and o_desc == o_resize and pix % 16 == 0 and pix >= o_desc + plan.desc.nbytes
    assert used == pix + plan.upload and total == pix + plan.nbytes
    flat = np.zeros(used, np.uint8)
    io.quad_fill(flat, plan)
    assert np.array_equal(flat[:plan.warp.nbytes].view(np.int32), plan.warp.reshape(-1))
    assert np.array_equal(flat[pix:pix + 97 * 211 * 3], np.asarray(scene).reshape(-1))
    with pytest.raises(ValueError, match="RGB"):
        io.quad_plan(scene.convert("L"), quads)
    with pytest.raises(ValueError, match="quad 0"):
        io.quad_plan(scene, [ROT15[::-1]])


def test_quad_plan_sends_a_crop_beyond_the_limits_through_a_fallback():
    """beyond `line_limits()`: resized on the device where the tiled resampler takes the factor, else rectified and resized on the host"""
    from tatt_amd import io
    lim, slim = io.line_limits(), io.scene_limits()
    tall = lim["rows"] + 20
    scene = _img(12, tall + 30, 300)
    quads = [AXIS, ((10, 5), (290, 8), (288, tall + 10), (12, tall + 5))]
    # windows 16 high: a crop of more than 256 rows shrinks by more than 16 : 1 -> the host fallback, uploaded behind the scene
    plan = io.quad_plan(scene, quads, LR, 32, True)
    assert tall > slim["down"] * 16 and len(plan.warp) == 1 and len(plan.resize) == 0 and len(plan.arrays) == 2
    wl = plan.lines[1].wl
    bw, bh = io.quad_size(quads[1])
    small = np.asarray(Image.fromarray(io.quad_rectify_host(scene, quads[1]), "RGB").resize((wl, 16), Image.BICUBIC))
    assert np.array_equal(plan.arrays[1], small) and plan.offsets[1] % 16 == 0 and plan.upload == plan.offsets[1] + -(-small.size // 16) * 16
    assert list(plan.desc[-1][:5]) == [plan.offsets[1], 16, wl, 16, wl] and plan.desc[-1][9] == 3 * wl
    # windows 32 high: the same crop is resized on the device: warp -> crop, resize -> (wl, 32), windows out of that
    plan = io.quad_plan(scene, quads, (32, 128), 64, True)
    wl = plan.lines[1].wl
    assert len(plan.warp) == 2 and len(plan.resize) == 1 and len(plan.arrays) == 1
    r = plan.resize[0]
    assert list(r[:4]) == [plan.warp[1][4], bh, bw, 3 * bw] and list(r[5:9]) == [32, wl, 3 * wl, 0] and r[4] % 16 == 0 and not r[9:].any()
    assert r[4] == plan.warp[1][4] + -(-bh * bw * 3 // 16) * 16 and plan.nbytes == r[4] + -(-32 * wl * 3 // 16) * 16
    assert list(plan.desc[-1][:5]) == [r[4], 32, wl, 32, wl]


def test_quad_paste_plan_layers_rows_and_offsets():
    from tatt_amd import io
    from tatt_amd.quads import QUAD_DESC
    quads = [ROT15, ((150, 60), (200, 60), (200, 90), (150, 90)), PERSXY, ROT90]          # 2 overlaps 0; 3 overlaps 0 and 2; 1 is alone
    assert io.quad_layers(quads) == [0, 0, 1, 2]
    lines = []
    for q in quads:
        wl, starts = io.line_plan(io.quad_size(q), LR, 32)
        lines.append(io.Line(wl, starts, sum(len(ln.starts) for ln in lines)))
    n = lines[-1].first + len(lines[-1].starts)
    bdesc, _, bbytes = io.blend_plan(lines, n, 32, 128, 2, "floor", 0)
    plan = io.quad_paste_plan(SIZE, quads, bdesc, bbytes, 2, 32, 3)
    assert plan.layers == [0, 0, 1, 2] and plan.order == [0, 1, 2, 3] and plan.counts == [2, 1, 1]
    assert plan.resize.shape == (5, 16) and plan.warp.shape == (4, QUAD_DESC)
    end = -(-bbytes // 16) * 16
    for k, q in enumerate(quads):
        bw, bh = io.quad_size(q)
        assert plan.rects[k] == end and end % 16 == 0
        assert list(plan.resize[1 + k][:9]) == [bdesc[k][6], 32, 2 * lines[k].wl, bdesc[k][7], end, 2 * bh, 2 * bw, 6 * bw, 0]
        end += -(-4 * bh * bw * 3 // 16) * 16
    assert plan.canvas_off == end and plan.pitch == 3 * 422 and plan.nbytes == end + 194 * plan.pitch
    assert list(plan.resize[0][:9]) == [0, 97, 211, 633, end, 194, 422, plan.pitch, 0]
    for r, k in enumerate(plan.order):
        bw, bh = io.quad_size(quads[k])
        x0, y0, x1, y1 = io.quad_bbox(quads[k])
        row = plan.warp[r]
        assert list(row[:10]) == [plan.rects[k], 2 * bh, 2 * bw, 6 * bw, end + 2 * y0 * plan.pitch + 6 * x0, 2 * (y1 - y0), 2 * (x1 - x0),
                                  plan.pitch, 3, 1]
        assert tuple(_words(row, i) for i in range(9)) == io.quad_matrices(quads[k], 2)[1] and not row[28:].any()
    swapped = io.quad_paste_plan(SIZE, [quads[2], quads[0]], bdesc[:2], bbytes, 2, 32, 0)  # an overlapping pair lands in two layers
    assert swapped.layers == [0, 1] and swapped.counts == [1, 1]
    with pytest.raises(ValueError, match="feather"):
        io.quad_paste_plan(SIZE, quads, bdesc, bbytes, 2, 32, -1)
    with pytest.raises(ValueError, match="lines for"):
        io.quad_paste_plan(SIZE, quads[:2], bdesc, bbytes, 2, 32, 0)


# ---- the C entry on host rows alone -------------------------------------------------------------------------------------------------
def test_quad_limits_need_no_gpu():
    from tatt_amd import io
    from tatt_amd.quads import QUAD_DESC
    lim = io.quad_limits()
    assert set(lim) == {"tile_h", "tile_w", "items", "side", "feather", "desc"}
    assert lim["tile_h"] * lim["tile_w"] == 256 and lim["desc"] == QUAD_DESC and lim["side"] >= 8192 and lim["feather"] >= 16
    assert lim["items"] >= io.scene_limits()["boxes"]


def test_warp_entry_return_codes_on_host_rows():
    from tatt_amd import io, ops
    from tatt_amd.quads import warp_row
    lim = io.quad_limits()
    sb, db = 70 * 450, 16 + 140 * 912
    m = io.quad_matrices(AXIS, 1)[0]

    def rc(rows, s=sb, d=db):
        host = np.ascontiguousarray(np.array(rows, np.int32))
        dummy = ctypes.c_void_p(host.ctypes.data)                   # (refused before a device pointer is read)
        return ops.LIB.tatt_warp_u8(dummy, s, dummy, dummy, len(rows), dummy, d, None)

    def row(**kw):
        base = dict(src=0, hs=70, ws=150, sp=450, dst=16, oh=140, ow=300, dp=912, f=0, mode=0)
        base.update({k: v for k, v in kw.items() if k in base})
        r = warp_row(*(base[k] for k in ("src", "hs", "ws", "sp", "dst", "oh", "ow", "dp", "f", "mode")), m)
        for i in range(28, 32):
            r[i] = kw.get("r%d" % i, 0)
        return r
    run = lambda r, **kw: rc([r], **kw)
    assert run(row(r28=1)) == 1 and run(row(r31=-1)) == 1 and run(row(f=-1)) == 1 and run(row(mode=2)) == 1 and run(row(mode=-1)) == 1
    assert rc([]) == 1 and run(row(), d=0) == 1 and run(row(), s=0) == 1
    assert run(row(hs=0)) == 2 and run(row(ow=0)) == 2 and run(row(f=lim["feather"] + 1)) == 2
    assert run(row(oh=lim["side"] + 1)) == 2 and run(row(ws=lim["side"] + 1)) == 2
    assert rc([row()] * (lim["items"] + 1)) == 2
    assert run(row(src=-1)) == 3 and run(row(sp=449)) == 3 and run(row(), s=sb - 1) == 3 and run(row(src=1)) == 3
    assert run(row(dst=-16)) == 3 and run(row(dp=899)) == 3 and run(row(), d=db - 13) == 3 and run(row(dst=32)) == 3
    # two faults in one row: the first test in the entry's order decides (reserved words, feather sign and mode; sides and feather; buffers)
    assert run(row(mode=2, hs=0)) == 1 and run(row(mode=-1, sp=449)) == 1 and run(row(r28=1, src=-1)) == 1 and run(row(f=-1, dp=899)) == 1
    assert run(row(mode=2, f=lim["feather"] + 1)) == 1 and run(row(hs=0, src=-1)) == 2 and run(row(f=lim["feather"] + 1, dst=-16)) == 2
    assert run(row(oh=lim["side"] + 1, dp=899)) == 2 and run(row(src=-1, dst=-16)) == 3


# ---- build --------------------------------------------------------------------------------------------------------------------------
def test_quads_source_is_built_without_contraction_and_exported():
    from tatt_amd import build, io
    from tatt_amd._lib import LIB
    assert "quads.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["quads.hip"]
    assert {"tatt_warp_u8", "tatt_quad_limits"} <= set(LIB.protos)
    for name in ("quad_check", "quad_size", "quad_matrices", "warp_u8_host", "quad_rectify_host", "quad_windows_host", "quad_compose_host",
                 "super_resolve_quads_host", "quad_plan", "quad_fill", "quad_paste_plan", "quad_limits"):
        assert callable(getattr(io, name)), name
