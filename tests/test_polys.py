"""CPU: the host specification of polygon text instances, curved text (tatt_amd/polys.py): the polygon check, what N = 2 must give (the
quad path, byte for byte), the paste's claim rule against exact rational geometry (no crack and no double painting at a seam), the
continuity of the sample across a seam, the feather, the host halves of the launches, the composition end to end and the return codes of
the C entry on host rows alone.  Exact integer arithmetic throughout: np.array_equal / ==, no tolerance but the 1 / 64 pixel band along
the OUTER boundary that the watertightness test leaves unasserted (and counts)."""
import ctypes
import itertools

import numpy as np
import pytest
from PIL import Image

from tests import pil_resample_ref as R

LR = (16, 64)
SIZE = (211, 97)                                                     # (Ws, Hs) of the scenes here
ONE = ((150, 60), (200, 62), (199, 88), (149, 86))                   # the quads of tests/test_quads_device_gpu.py
THREE = ((20, 10), (140, 30), (138, 46), (18, 26))
PERSX = ((30, 10), (180, 25), (175, 70), (35, 90))
ARC = ((10, 40), (40, 22), (75, 18), (110, 30), (104, 50), (74, 38), (44, 42), (20, 58))                               # N = 4
SCURVE = ((10, 30), (45, 20), (85, 28), (125, 40), (165, 34), (168, 52), (123, 58), (82, 46), (47, 39), (14, 48))      # N = 5
# N = 8 around a ring: seven strips of 40 degrees (a horseshoe), and of 55 degrees (385 in all: the last strip runs into the first)
HORSESHOE = ((24, 79), (11, 55), (15, 28), (36, 10), (64, 10), (85, 28), (89, 55), (76, 79),
             (64, 65), (72, 52), (69, 37), (58, 27), (42, 27), (31, 37), (28, 52), (36, 65))
CROSSING = ((24, 79), (10, 45), (30, 13), (67, 12), (89, 41), (78, 76), (43, 87), (14, 65),
            (30, 57), (46, 70), (66, 64), (72, 44), (59, 28), (39, 29), (28, 46), (36, 65))


def _img(seed, hs, ws, kind=1):
    return Image.fromarray(R.make_image(np.random.default_rng(seed), hs, ws, kind), "RGB")


def _as_poly(quad):
    return tuple(quad)                                               # a quad IS the polygon with N = 2: t_0, t_1, b_1, b_0


# ---- the check ----------------------------------------------------------------------------------------------------------------------
def test_poly_check_accepts_and_refuses():
    from tatt_amd import io
    ok = io.poly_check(SIZE, [ARC, SCURVE, ONE, HORSESHOE])
    assert ok == [ARC, SCURVE, ONE, HORSESHOE]
    assert io.poly_check(SIZE, [[list(p) for p in ARC]]) == [ARC] and io.poly_check(SIZE, []) == []
    assert io.poly_strips(ARC) == [(ARC[0], ARC[1], ARC[6], ARC[7]), (ARC[1], ARC[2], ARC[5], ARC[6]), (ARC[2], ARC[3], ARC[4], ARC[5])]
    assert io.poly_size(ARC) == (107, 21) and io.poly_columns(ARC) == ([35, 35, 37], [0, 35, 70]) and io.poly_bbox(ARC) == (10, 18, 110, 58)
    bad = [(ARC[:7], None),                                          # an odd point count
           (ARC[:2], None),                                          # two points
           (HORSESHOE[:8] + ((70, 70),) + ((66, 67),) + HORSESHOE[8:], None),               # 18 points
           (ARC[:3] + ((110.0, 30),) + ARC[4:], None),               # a float
           (ARC[:3] + ((110, True),) + ARC[4:], None),               # a bool
           (ARC[:3] + ((212, 30),) + ARC[4:], None),                 # leaves the image
           (ARC[::-1], 0),                                           # counter-clockwise
           (ARC[:2] + ((60, 40),) + ARC[3:], 1),                     # strip 1 is not convex: t_2 below the line b_1 b_2
           (((20, 10), (60, 10), (120, 10), (120, 30), (60, 40), (20, 71)), 0),              # strip 0: 61 against 30, beyond 2 : 1
           (((20, 10), (21, 10), (60, 10), (60, 30), (21, 30), (20, 30)), 0),                # strip 0 takes one column
           (((20, 10), (40, 10), (60, 10), (60, 13), (40, 13), (20, 13)), None),             # 3 high
           (CROSSING, 0)]                                            # strip 6 runs into strip 0
    for poly, strip in bad:
        with pytest.raises(ValueError, match="polygon 1" + ("" if strip is None else r".*strip %d" % strip)):
            io.poly_check(SIZE, [ARC, poly])
    with pytest.raises(ValueError, match="crosses itself"):
        io.poly_check(SIZE, [CROSSING])
    with pytest.raises(ValueError, match="at most"):
        io.poly_check(SIZE, [ARC, SCURVE], dict(io.scene_limits(), boxes=1))
    with pytest.raises(ValueError, match="image"):
        io.poly_check((0, 97), [])


# ---- N = 2 is the quad path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1, 2))
@pytest.mark.parametrize("quad", (ONE, THREE, PERSX), ids=("one", "three", "persx"))
def test_four_points_give_what_the_quad_path_gives(quad, scale):
    from tatt_amd import io
    scene = _img(3, 97, 211)
    poly = _as_poly(quad)
    assert io.poly_check(SIZE, [poly]) == io.quad_check(SIZE, [quad]) and io.poly_size(poly) == io.quad_size(quad)
    m_rect, m_paste, bbox = io.quad_matrices(quad, scale)
    maps = io.poly_matrices(poly, scale)
    bw, bh = io.quad_size(quad)
    assert maps.rect == [m_rect] and maps.paste == [m_paste] and maps.bbox == bbox == io.poly_bbox(poly) and maps.seams == []
    assert maps.widths == [bw] and maps.bh == bh and maps.scale == scale
    assert np.array_equal(io.poly_rectify_host(scene, poly), io.quad_rectify_host(scene, quad))
    line = R.make_image(np.random.default_rng(5), scale * bh, scale * bw, 1)
    oh, ow = scale * (bbox[3] - bbox[1]), scale * (bbox[2] - bbox[0])
    before = np.random.default_rng(6).integers(0, 256, (oh, ow, 3), dtype=np.uint8)
    for feather in (0, 1, 5):
        want = io.warp_u8_host(line, m_paste, oh, ow, before.copy(), feather)
        got = io.poly_paste_host(line, maps, before.copy(), feather)
        assert np.array_equal(got, want), (feather, int((got != want).sum()))
        assert not np.array_equal(got, before)


def test_quad_plans_are_the_poly_plans_of_four_point_regions():
    """the five quads of tests/test_quads.py as quads and as polygons of four points: the same window plan, the same paste plan up to
    the rows of the paste launch, whose shared words and matrices agree"""
    from tatt_amd import io
    from tests.test_quads import FIVE
    scene = _img(3, 97, 211)
    polys = [_as_poly(q) for q in FIVE]
    a, b = io.quad_plan(scene, FIVE, LR, 32, True), io.poly_plan(scene, polys, LR, 32, True)
    for name in ("offsets", "lines", "upload", "nbytes", "out_floats"):
        assert getattr(a, name) == getattr(b, name), name
    for name in ("warp", "resize", "desc"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert len(a.arrays) == len(b.arrays) and all(np.array_equal(x, y) for x, y in zip(a.arrays, b.arrays))
    lines = a.lines
    n = lines[-1].first + len(lines[-1].starts)
    for scale in (1, 2):
        bdesc, _, bbytes = io.blend_plan(lines, n, 16 * scale, 64 * scale, scale, "floor", 0)
        a = io.quad_paste_plan(SIZE, FIVE, bdesc, bbytes, scale, 16 * scale, 3)
        b = io.poly_paste_plan(SIZE, polys, bdesc, bbytes, scale, 16 * scale, 3)
        for name in ("layers", "order", "counts", "rects", "canvas_off", "pitch", "nbytes"):
            assert getattr(a, name) == getattr(b, name), (scale, name)
        assert np.array_equal(a.resize, b.resize)
        assert len(a.warp) == len(b.items) == len(b.strips) == len(FIVE)
        for r, (row, item) in enumerate(zip(a.warp, b.items)):
            assert list(row[:9]) == list(item[:9]) and list(item[9:11]) == [r, 1], (scale, r)
            assert list(row[10:28]) == list(b.strips[r][2:20]), (scale, r)


# ---- the claim rule against exact rational geometry ---------------------------------------------------------------------------------
def _cross(a, b, p):
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])


def _geometry(poly, scale):
    """the polygon on the scaled bounding box in HALF-pixel units (a pixel centre is (2 j + 1, 2 i + 1)): all integers.  -> (inside, near):
    inside[i, j]: the centre lies in the closed union of the strips; near[i, j]: it lies within 1 / 64 pixel of the OUTER boundary (the top
    and bottom polylines and the two end seams).  Point-in-quad by the signs of four cross products; the distance to a segment by
    comparing squares of integers."""
    from tatt_amd import io
    x0, y0, x1, y1 = io.poly_bbox(poly)
    pts = [(2 * scale * (x - x0), 2 * scale * (y - y0)) for x, y in poly]
    n = len(pts) // 2
    strips = io.poly_strips(pts)
    outer = [(pts[k], pts[k + 1]) for k in range(n - 1)] + [(pts[n - 1], pts[n])] + [(pts[k], pts[k + 1]) for k in range(n, 2 * n - 1)] + [
        (pts[2 * n - 1], pts[0])]
    oh, ow = scale * (y1 - y0), scale * (x1 - x0)
    inside, near = np.zeros((oh, ow), bool), np.zeros((oh, ow), bool)
    for i in range(oh):
        for j in range(ow):
            p = (2 * j + 1, 2 * i + 1)
            inside[i, j] = any(all(_cross(s[e], s[(e + 1) % 4], p) >= 0 for e in range(4)) for s in strips)
            for a, b in outer:                                       # dist^2 <= (2 / 64)^2 half-pixel units, i.e. 1024 dist^2 <= 1
                ab2 = (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
                t = (p[0] - a[0]) * (b[0] - a[0]) + (p[1] - a[1]) * (b[1] - a[1])
                if t <= 0:
                    close = 1024 * ((p[0] - a[0]) ** 2 + (p[1] - a[1]) ** 2) <= 1
                elif t >= ab2:
                    close = 1024 * ((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2) <= 1
                else:
                    close = 1024 * _cross(a, b, p) ** 2 <= ab2
                if close:
                    near[i, j] = True
                    break
    return inside, near


@pytest.fixture(scope="module", params=[(ARC, 1), (ARC, 2), (SCURVE, 1), (SCURVE, 2)], ids=("arc-1", "arc-2", "scurve-1", "scurve-2"))
def pasted(request):
    """a line of constant 255 pasted onto zeros, feather 0 -> (poly, scale, maps, the painted mask, inside, near)"""
    from tatt_amd import io
    poly, scale = request.param
    maps = io.poly_matrices(poly, scale)
    bw, bh = io.poly_size(poly)
    line = np.full((scale * bh, scale * bw, 3), 255, np.uint8)
    x0, y0, x1, y1 = maps.bbox
    dst = io.poly_paste_host(line, maps, np.zeros((scale * (y1 - y0), scale * (x1 - x0), 3), np.uint8), 0)
    assert set(np.unique(dst)) == {0, 255} and np.array_equal(dst[:, :, 0], dst[:, :, 1]) and np.array_equal(dst[:, :, 0], dst[:, :, 2])
    return poly, scale, maps, dst[:, :, 0] == 255, *_geometry(poly, scale)


def test_paste_is_watertight_against_exact_geometry(pasted):
    from tatt_amd import io
    poly, scale, maps, painted, inside, near = pasted
    print("%d of %d pixels lie within 1 / 64 pixel of the outer boundary" % (near.sum(), near.size))
    assert near.sum() <= 0.02 * near.size
    assert painted[inside & ~near].all(), int((~painted & inside & ~near).sum())           # no crack: the seams get no exemption
    assert not painted[~inside & ~near].any(), int((painted & ~inside & ~near).sum())
    assert painted.any() and not painted.all()
    # every strip painted alone: pairwise disjoint masks, their union the whole mask
    line = np.full((maps.scale * maps.bh, maps.scale * sum(maps.widths), 3), 255, np.uint8)
    alone = [io.poly_paste_host(line, maps, np.zeros(painted.shape + (3,), np.uint8), 0, strips=(k,))[:, :, 0] == 255
             for k in range(len(maps.paste))]
    assert all(m.any() for m in alone)
    for a, b in itertools.combinations(range(len(alone)), 2):
        assert not (alone[a] & alone[b]).any(), (a, b)
    assert np.array_equal(np.logical_or.reduce(alone), painted)
    owner = io.poly_owner_host(maps)
    assert all(np.array_equal(owner == k, m) for k, m in enumerate(alone)) and np.array_equal(owner >= 0, painted)


@pytest.mark.parametrize("poly,scale", ((ARC, 1), (ARC, 2), (SCURVE, 1)), ids=("arc-1", "arc-2", "scurve-1"))
def test_the_sample_is_continuous_across_a_seam(poly, scale):
    """a horizontal ramp, value = column: across a seam the step between horizontal neighbours is no larger than inside the two strips"""
    from tatt_amd import io
    maps = io.poly_matrices(poly, scale)
    bw, bh = io.poly_size(poly)
    assert scale * bw <= 256
    line = np.broadcast_to(np.arange(scale * bw, dtype=np.uint8)[None, :, None], (scale * bh, scale * bw, 3))
    x0, y0, x1, y1 = maps.bbox
    dst = io.poly_paste_host(line, maps, np.zeros((scale * (y1 - y0), scale * (x1 - x0), 3), np.uint8), 0)[:, :, 0].astype(int)
    owner = io.poly_owner_host(maps)
    a, b = owner[:, :-1], owner[:, 1:]
    step = np.abs(dst[:, 1:] - dst[:, :-1])
    for s in range(1, len(maps.paste)):                              # seam s lies between strip s - 1 and strip s
        across = ((a == s - 1) & (b == s)) | ((a == s) & (b == s - 1))
        within = (a == b) & ((a == s - 1) | (a == s))
        assert across.sum() >= 4 and within.any()
        assert step[across].max() <= step[within].max() + 1, (s, int(step[across].max()), int(step[within].max()))


def test_the_feather_fades_the_outer_sides_and_no_seam():
    """255 over 0 with F = 3: a painted byte tells its weight, (2 a 255 + D) // (2 D).  A pixel beside an interior seam and F + 2 pixels
    or more from the outer boundary (the line is at least as dense as the canvas: more than F line pixels) has a = D and equals its
    feather-0 byte; a pixel whose centre lies within 1 / 8 pixel of the outer boundary (under half a line pixel) has a = 1."""
    from tatt_amd import io
    F, D = 3, 4
    poly, scale = ARC, 2
    maps = io.poly_matrices(poly, scale)
    bw, bh = io.poly_size(poly)
    line = np.full((scale * bh, scale * bw, 3), 255, np.uint8)
    x0, y0, x1, y1 = maps.bbox
    oh, ow = scale * (y1 - y0), scale * (x1 - x0)
    plain = io.poly_paste_host(line, maps, np.zeros((oh, ow, 3), np.uint8), 0)[:, :, 0]
    soft = io.poly_paste_host(line, maps, np.zeros((oh, ow, 3), np.uint8), F)[:, :, 0]
    owner = io.poly_owner_host(maps)
    assert np.array_equal(soft > 0, owner >= 0) and set(np.unique(soft)) == {0} | {(2 * a * 255 + D) // (2 * D) for a in range(1, D + 1)}
    pts = [(scale * (x - x0), scale * (y - y0)) for x, y in poly]
    n = len(pts) // 2
    outer = [(pts[k], pts[(k + 1) % (2 * n)]) for k in range(2 * n) if k not in (n - 1, 2 * n - 1)] + [(pts[n - 1], pts[n]), (pts[2 * n - 1], pts[0])]

    def dist(i, j):
        best = float("inf")
        for (ax, ay), (bx, by) in outer:
            px, py, dx, dy = j + 0.5 - ax, i + 0.5 - ay, bx - ax, by - ay
            t = min(1.0, max(0.0, (px * dx + py * dy) / (dx * dx + dy * dy)))
            best = min(best, ((px - t * dx) ** 2 + (py - t * dy) ** 2) ** 0.5)
        return best
    seam = np.zeros((oh, ow), bool)
    seam[:, :-1] |= (owner[:, :-1] >= 0) & (owner[:, 1:] >= 0) & (owner[:, :-1] != owner[:, 1:])
    seam[:, 1:] |= seam[:, :-1]
    deep = edge = 0
    for i, j in zip(*np.nonzero(owner >= 0)):
        d = dist(i, j)
        if seam[i, j] and d >= F + 2:
            assert soft[i, j] == plain[i, j] == 255, (i, j)
            deep += 1
        if d <= 0.125:
            assert soft[i, j] == (2 * 255 + D) // (2 * D), (i, j, soft[i, j])
            edge += 1
    assert deep >= 20 and edge >= 20, (deep, edge)


# ---- the host halves of the launches ------------------------------------------------------------------------------------------------
def _words(row, k, base):
    lo, hi = int(row[base + 2 * k]) & 0xFFFFFFFF, int(row[base + 2 * k + 1])
    return (hi << 32) | lo


def test_poly_plan_one_warp_row_per_strip_and_fill():
    from tatt_amd import io
    from tatt_amd.quads import QUAD_DESC
    scene = _img(11, 97, 211)
    polys = [ARC, ONE, SCURVE]
    plan = io.poly_plan(scene, polys, LR, 32, True)
    _, lines = io.poly_windows_host(scene, polys, LR, 32, True)
    assert plan.lines == lines and plan.polys == polys and len(plan.arrays) == 1 and plan.upload == -(-97 * 211 * 3 // 16) * 16
    assert plan.warp.shape == (3 + 1 + 4, QUAD_DESC) and plan.resize.shape[0] == 0
    assert plan.desc.shape[0] == sum(len(ln.starts) for ln in lines)
    off, r = plan.upload, 0
    for k, poly in enumerate(polys):
        bw, bh = io.poly_size(poly)
        maps = io.poly_matrices(poly, 1)
        widths, starts = io.poly_columns(poly)
        assert off % 16 == 0
        for n, (wk, uk) in enumerate(zip(widths, starts)):           # the strips side by side in ONE crop of pitch 3 bw
            row = plan.warp[r]
            assert list(row[:10]) == [0, 97, 211, 633, off + 3 * uk, bh, wk, 3 * bw, 0, 0], (k, n)
            assert tuple(_words(row, i, 10) for i in range(9)) == maps.rect[n] and not row[28:].any()
            r += 1
        for x, d in zip(lines[k].starts, plan.desc[lines[k].first:]):
            assert list(d[:8]) == [off, bh, bw, 16, lines[k].wl, x, 64, 1] and d[9] == 3 * bw
        off += -(-bh * bw * 3 // 16) * 16
    assert plan.nbytes == off and plan.out_floats == plan.desc.shape[0] * 4 * 16 * 64
    o_warp, o_resize, o_desc, pix, used, total = io.poly_fill(None, plan)
    assert (o_warp, o_resize) == (0, plan.warp.nbytes) and o_desc == o_resize and pix == o_desc + -(-plan.desc.nbytes // 16) * 16
    assert used == pix + plan.upload and total == pix + plan.nbytes
    flat = np.zeros(used, np.uint8)
    io.poly_fill(flat, plan)
    assert np.array_equal(flat[:plan.warp.nbytes].view(np.int32), plan.warp.reshape(-1))
    assert np.array_equal(flat[pix:pix + 97 * 211 * 3], np.asarray(scene).reshape(-1))
    with pytest.raises(ValueError, match="RGB"):
        io.poly_plan(scene.convert("L"), polys)
    with pytest.raises(ValueError, match="polygon 0"):
        io.poly_plan(scene, [ARC[::-1]])


def test_poly_plan_sends_a_crop_beyond_the_limits_through_a_fallback():
    from tatt_amd import io
    lim, slim = io.line_limits(), io.scene_limits()
    tall = lim["rows"] + 20
    scene = _img(12, tall + 30, 300)
    big = ((10, 5), (150, 6), (290, 8), (288, tall + 10), (150, tall + 8), (12, tall + 5))                  # N = 3, two strips
    polys = [ARC, big]
    bw, bh = io.poly_size(big)
    # windows 16 high: the crop shrinks by more than 16 : 1 -> rectified and resized on the host, uploaded behind the scene
    plan = io.poly_plan(scene, polys, LR, 32, True)
    assert bh > lim["rows"] and tall > slim["down"] * 16 and len(plan.warp) == 3 and len(plan.resize) == 0 and len(plan.arrays) == 2
    wl = plan.lines[1].wl
    small = np.asarray(Image.fromarray(io.poly_rectify_host(scene, big), "RGB").resize((wl, 16), Image.BICUBIC))
    assert np.array_equal(plan.arrays[1], small) and plan.offsets[1] % 16 == 0
    assert list(plan.desc[-1][:5]) == [plan.offsets[1], 16, wl, 16, wl] and plan.desc[-1][9] == 3 * wl
    # windows 32 high: the crop is resized on the device
    plan = io.poly_plan(scene, polys, (32, 128), 64, True)
    wl = plan.lines[1].wl
    assert len(plan.warp) == 5 and len(plan.resize) == 1 and len(plan.arrays) == 1
    r = plan.resize[0]
    assert list(r[:4]) == [plan.warp[3][4], bh, bw, 3 * bw] and list(r[5:9]) == [32, wl, 3 * wl, 0] and r[4] % 16 == 0
    assert plan.warp[4][4] == plan.warp[3][4] + 3 * plan.warp[3][6] and list(plan.desc[-1][:5]) == [r[4], 32, wl, 32, wl]


def test_poly_paste_plan_layers_rows_and_offsets():
    from tatt_amd import io
    from tatt_amd.polys import POLY_DESC, POLY_STRIP_DESC
    polys = [ARC, ONE, SCURVE]                                       # SCURVE's bounding box meets ARC's; ONE is alone
    assert io.poly_layers(polys) == [0, 0, 1]
    lines = []
    for p in polys:
        wl, starts = io.line_plan(io.poly_size(p), LR, 32)
        lines.append(io.Line(wl, starts, sum(len(ln.starts) for ln in lines)))
    n = lines[-1].first + len(lines[-1].starts)
    bdesc, _, bbytes = io.blend_plan(lines, n, 32, 128, 2, "floor", 0)
    plan = io.poly_paste_plan(SIZE, polys, bdesc, bbytes, 2, 32, 3)
    assert plan.layers == [0, 0, 1] and plan.order == [0, 1, 2] and plan.counts == [2, 1]
    assert plan.resize.shape == (4, 16) and plan.items.shape == (3, POLY_DESC) and plan.strips.shape == (3 + 1 + 4, POLY_STRIP_DESC)
    end = -(-bbytes // 16) * 16
    for k, p in enumerate(polys):
        bw, bh = io.poly_size(p)
        assert plan.rects[k] == end and end % 16 == 0
        assert list(plan.resize[1 + k][:9]) == [bdesc[k][6], 32, 2 * lines[k].wl, bdesc[k][7], end, 2 * bh, 2 * bw, 6 * bw, 0]
        end += -(-4 * bh * bw * 3 // 16) * 16
    assert plan.canvas_off == end and plan.pitch == 3 * 422 and plan.nbytes == end + 194 * plan.pitch
    assert list(plan.resize[0][:9]) == [0, 97, 211, 633, end, 194, 422, plan.pitch, 0]
    first = 0
    for r, k in enumerate(plan.order):
        bw, bh = io.poly_size(polys[k])
        x0, y0, x1, y1 = io.poly_bbox(polys[k])
        maps = io.poly_matrices(polys[k], 2)
        widths, starts = io.poly_columns(polys[k])
        item = plan.items[r]
        assert list(item[:11]) == [plan.rects[k], 2 * bh, 2 * bw, 6 * bw, end + 2 * y0 * plan.pitch + 6 * x0, 2 * (y1 - y0), 2 * (x1 - x0),
                                   plan.pitch, 3, first, len(widths)] and not item[11:].any()
        for s in range(len(widths)):
            row = plan.strips[first + s]
            assert list(row[:2]) == [2 * starts[s], 2 * widths[s]]
            vals = tuple(_words(row, i, 2) for i in range(15))
            assert vals[:9] == maps.paste[s]
            assert vals[9:12] == (maps.seams[s - 1] if s else (0, 0, 0)) and vals[12:] == (maps.seams[s] if s < len(widths) - 1 else (0, 0, 0))
        first += len(widths)
    swapped = io.poly_paste_plan(SIZE, [polys[2], polys[0]], bdesc[:2], bbytes, 2, 32, 0)
    assert swapped.layers == [0, 1] and swapped.counts == [1, 1]
    with pytest.raises(ValueError, match="feather"):
        io.poly_paste_plan(SIZE, polys, bdesc, bbytes, 2, 32, -1)
    with pytest.raises(ValueError, match="lines for"):
        io.poly_paste_plan(SIZE, polys[:2], bdesc, bbytes, 2, 32, 0)


def test_seam_edge_functions_are_exact_and_signed_along_the_reading_direction():
    from tatt_amd import io
    for poly, scale in ((ARC, 1), (SCURVE, 2)):
        maps = io.poly_matrices(poly, scale)
        n = len(poly) // 2
        x0, y0 = maps.bbox[:2]
        assert len(maps.seams) == n - 2
        for s, (A, B, C) in enumerate(maps.seams, start=1):
            at = lambda p: A * 2 * scale * (p[0] - x0) + B * 2 * scale * (p[1] - y0) + C       # a scene point in half-pixel units
            assert at(poly[s]) == 0 and at(poly[2 * n - 1 - s]) == 0                            # through t_s and b_s, exactly
            assert at(poly[s + 1]) > 0 and at(poly[2 * n - 2 - s]) > 0 and at(poly[s - 1]) < 0 and at(poly[2 * n - s]) < 0


# ---- the composition ----------------------------------------------------------------------------------------------------------------
def test_super_resolve_polys_host_end_to_end():
    from tatt_amd import io
    scene = _img(13, 97, 211)
    polys = [ARC, ONE, SCURVE]
    seen = []

    def nearest(stack):
        seen.append(stack.shape[0])
        return stack[:, :3].repeat_interleave(2, 2).repeat_interleave(2, 3)
    out = io.super_resolve_polys_host(scene, polys, nearest, LR, 32, True)
    _, lines = io.poly_windows_host(scene, polys, LR, 32, True)
    assert seen == [len(ln.starts) for ln in lines]
    assert out.mode == "RGB" and out.size == (422, 194)
    up = np.asarray(scene.resize((422, 194), Image.BICUBIC))
    got = np.asarray(out)
    outside = np.ones((194, 422), bool)
    for p in polys:
        x0, y0, x1, y1 = io.poly_bbox(p)
        outside[2 * y0:2 * y1, 2 * x0:2 * x1] = False
        assert not np.array_equal(got[2 * y0:2 * y1, 2 * x0:2 * x1], up[2 * y0:2 * y1, 2 * x0:2 * x1])
    assert np.array_equal(got[outside], up[outside])
    # no polygons: the plain up-scale, at the scale the caller names
    assert np.array_equal(np.asarray(io.super_resolve_polys_host(scene, [], nearest, LR, 32, True, scale=2)), up)
    with pytest.raises(ValueError, match="no polygons"):
        io.super_resolve_polys_host(scene, [], nearest)


# ---- the C entry on host rows alone -------------------------------------------------------------------------------------------------
def test_poly_limits_need_no_gpu():
    from tatt_amd import io
    from tatt_amd.polys import POLY_DESC, POLY_MAX_POINTS, POLY_STRIP_DESC
    lim = io.poly_limits()
    assert set(lim) == {"tile_h", "tile_w", "items", "side", "feather", "desc", "strip_desc", "strips"}
    assert lim["tile_h"] * lim["tile_w"] == 256 and lim["desc"] == POLY_DESC and lim["strip_desc"] == POLY_STRIP_DESC
    assert lim["strips"] >= POLY_MAX_POINTS // 2 - 1 and lim["items"] >= io.scene_limits()["boxes"]
    assert lim["side"] == io.quad_limits()["side"] and lim["feather"] == io.quad_limits()["feather"]


def test_poly_paste_entry_return_codes_on_host_rows():
    from tatt_amd import io, ops
    from tatt_amd.polys import poly_item_row, poly_strip_row
    lim = io.poly_limits()
    sb, db = 70 * 450, 16 + 140 * 912
    maps = io.poly_matrices(ARC, 2)
    strips = [poly_strip_row(0, 50, maps.paste[0], None, maps.seams[0]), poly_strip_row(50, 50, maps.paste[1], maps.seams[0], maps.seams[1]),
              poly_strip_row(100, 50, maps.paste[2], maps.seams[1], None)]

    def rc(items, table=strips, s=sb, d=db, n_strips=None):
        host = np.ascontiguousarray(np.array(items, np.int32))
        tab = np.ascontiguousarray(np.array(table, np.int32))
        dummy = ctypes.c_void_p(host.ctypes.data)                   # (refused before a device pointer is read)
        return ops.LIB.tatt_poly_paste_u8(dummy, s, dummy, dummy, len(items), dummy, ctypes.c_void_p(tab.ctypes.data),
                                          len(table) if n_strips is None else n_strips, dummy, d, None)

    def item(**kw):
        base = dict(src=0, hs=70, ws=150, sp=450, dst=16, oh=140, ow=300, dp=912, f=0, first=0, count=3)
        base.update({k: v for k, v in kw.items() if k in base})
        r = poly_item_row(*(base[k] for k in ("src", "hs", "ws", "sp", "dst", "oh", "ow", "dp", "f", "first", "count")))
        for i in range(11, 16):
            r[i] = kw.get("r%d" % i, 0)
        return r
    run = lambda r, **kw: rc([r], **kw)
    assert run(item(r11=1)) == 1 and run(item(r15=-1)) == 1 and run(item(f=-1)) == 1
    assert rc([]) == 1 and run(item(), d=0) == 1 and run(item(), s=0) == 1 and run(item(), n_strips=0) == 1
    assert run(item(hs=0)) == 2 and run(item(ow=0)) == 2 and run(item(f=lim["feather"] + 1)) == 2
    assert run(item(oh=lim["side"] + 1)) == 2 and run(item(ws=lim["side"] + 1)) == 2
    assert run(item(count=0)) == 2 and run(item(count=lim["strips"] + 1)) == 2
    assert rc([item()] * (lim["items"] + 1)) == 2
    assert run(item(ws=149, sp=450)) == 2                            # the last strip's columns leave the line
    assert run(item(src=-1)) == 3 and run(item(sp=449)) == 3 and run(item(), s=sb - 1) == 3 and run(item(src=1)) == 3
    assert run(item(dst=-16)) == 3 and run(item(dp=899)) == 3 and run(item(), d=db - 13) == 3 and run(item(dst=32)) == 3
    assert run(item(first=1)) == 4 and run(item(first=-1)) == 4 and run(item(), n_strips=2) == 4 and run(item(first=3, count=1)) == 4
    # two faults in one item: the first test in the entry's order decides (reserved words and feather sign; sides, feather and strip
    # count; buffers; the strip table; the strips' columns)
    assert run(item(r11=1, count=0)) == 1 and run(item(f=-1, hs=0)) == 1 and run(item(f=-1, src=-1)) == 1
    assert run(item(count=0, src=-1)) == 2 and run(item(count=lim["strips"] + 1, dp=899)) == 2 and run(item(hs=0, first=-1)) == 2
    assert run(item(count=0, first=-1)) == 2 and run(item(f=lim["feather"] + 1, dst=-16)) == 2
    assert run(item(sp=449, first=1)) == 3 and run(item(ws=149, src=-1)) == 3 and run(item(ws=149, first=1)) == 4


# ---- build --------------------------------------------------------------------------------------------------------------------------
def test_polys_source_is_built_without_contraction_and_exported():
    from tatt_amd import build, io
    from tatt_amd._lib import LIB
    assert "polys.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["polys.hip"]
    assert {"tatt_poly_paste_u8", "tatt_poly_limits"} <= set(LIB.protos)
    for name in ("poly_check", "poly_strips", "poly_size", "poly_bbox", "poly_matrices", "poly_rectify_host", "poly_paste_host",
                 "poly_windows_host", "poly_layers", "poly_compose_host", "super_resolve_polys_host", "poly_limits", "poly_plan",
                 "poly_fill", "poly_paste_plan"):
        assert callable(getattr(io, name)), name
    from tatt_amd.infer import SuperResolver
    assert callable(SuperResolver.scene_polys) and callable(io.DeviceCollator.poly_windows) and callable(io.DeviceExporter.scene_polys)
