"""Scene images with POLYGON text instances: curved text (csrc/polys.hip; `DeviceCollator.poly_windows`, `DeviceExporter.scene_polys`,
`infer.SuperResolver.scene_polys`).

Detectors of curved text (DBNet, the CTW1500 and Total-Text conventions) give a polygon of 2 N points per instance: N points
t_0 .. t_{N-1} along the top of the text in reading direction, then N points b_{N-1} .. b_0 back along the bottom (clockwise with y
down; N = 2 is a quad of `tatt_amd/quads.py`).  The polygon is cut into N - 1 STRIPS, strip k the quad (t_k, t_{k+1}, b_{k+1}, b_k);
SEAM s is the segment t_s b_s.  Every strip gets the projective map `quads.py` derives, so the polygon is straightened piecewise: strip k
fills w_k columns of the (bh, bw) crop, side by side, and the crop is a text line like any other.  The finished line is warped back
strip by strip into the polygon's bounding box of the up-scaled picture.

This module is the specification on the host, pure Python / numpy / PIL: integer plans derived in `fractions.Fraction`, every pixel in
64-bit integers, so the device path equals it byte for byte.
* `poly_check` / `poly_strips` / `poly_size` / `poly_columns` / `poly_bbox`: what a list of polygons must satisfy and its sizes:
  bh = max over the seams of _r(|t_s b_s|^2), w_k = _r(max(|t_k t_{k+1}|^2, |b_k b_{k+1}|^2)), U_k = w_0 + .. + w_{k-1}, bw = sum w_k.
* `poly_matrices`: per strip the two integer matrices (rectify, paste), the bounding box, the edge function of every interior seam.
* `poly_rectify_host` / `poly_paste_host` / `poly_owner_host`: the crop, the paste, which strip paints which pixel.
* `poly_windows_host` / `poly_layers` / `poly_compose_host` / `super_resolve_polys_host`: the composition.
* `poly_limits` / `poly_plan` / `poly_fill` / `poly_paste_plan`: the host halves of the launches (tatt_warp_u8 mode 0 with one row per
  strip, tatt_resize_u8, tatt_scene_windows, tatt_poly_paste_u8).

A quad is the polygon of four points, so what `tatt_amd/quads.py` offers under its `quad_*` names runs the bodies of this module with the
quad's wording (`_QUAD`): `_check`, `_maps`, `_window_plan`, `_paste_front`.  The projective arithmetic and the pixel rule on arrays
(`_sample_host`) live in `quads.py`.

Rectifying is `warp_u8_host` (mode 0) per strip with the strip's m_rect into columns [U_k, U_k + w_k) of the crop; the source is the
scene, so no strip needs its neighbour.

The paste is stated per destination pixel (i, j) of the polygon's bounding box on the up-scaled canvas, J = 2 j + 1, I = 2 i + 1 (the
pixel centre in half-pixel units, local to the box).  Seam s = 1 .. N - 2 has the exact edge function
    E_s(J, I) = A J + B I + C                  (int64; no rounding; E_s >= 0 on the side of strip s, further along the reading direction)
and strip k the nine integers m of its m_paste, applied as `quads.py` states (X, Y, Wd; gx = floor(256 X / Wd), gy = floor(256 Y / Wd)),
gx local to the strip.  The strips are tried in order k = 0, 1, ..; the FIRST strip that claims the pixel paints it, a pixel no strip
claims is left as it is.  Strip k claims the pixel iff
    E_k >= 0 (k >= 1),   E_{k+1} < 0 (k <= N - 3),   Wd > 0,   0 <= gy < 256 H,   gx >= 0 (k = 0),   gx < 256 scale w_k (k = N - 2)
for the (H, W) = (scale bh, scale bw) line.  The interior seams are decided by the edge functions alone, and two neighbouring strips
evaluate the same integers for the seam they share: every pixel between the outer sides belongs to exactly one strip (no crack, no pixel
painted twice); the outer sides keep the quad kernel's own test.  The sample is taken from the WHOLE line:
    gxg = gx + 256 scale U_k;   fx = gxg - 128, fy = gy - 128;   x0 = fx >> 8, ax = fx & 255 (fy alike)
with the four taps clamped to the line rectangle (across a seam a tap reads the neighbouring strip's columns, not a replicated edge); the
bilinear sum and its rounding are `warp_u8_host`'s.  The feather distance is measured to the nearest side of the whole line,
    xi = clamp(gxg >> 8, 0, W - 1), yi = gy >> 8, d = min(xi, W - 1 - xi, yi, H - 1 - yi)
(nothing fades at a seam) and the blend is `warp_u8_host`'s.  A polygon with N = 2 gets the bytes `warp_u8_host` gives its quad.
"""
from __future__ import annotations

import numbers
from collections import namedtuple
from fractions import Fraction

from .lines import Line, _compose_front, _line_takes, _region_windows_host, _scale_check, _super_resolve_boxes_host, line_limits, line_plan
from .quads import (QUAD_DESC, QUAD_MAX_TAPER, _adjugate, _d2, _diag, _homography, _integer, _mul, _r, _sample_host, _warp_coords, _words,
                    quad_bbox, quad_fill, quad_limits, warp_row, warp_u8_host)
from .scene import RESIZE_DESC, SCENE_DESC, SCENE_MIN_SIDE, _paste_order, _up, scene_layers, scene_limits

POLY_MIN_POINTS = 4       # N = 2: a quad
POLY_MAX_POINTS = 16      # N = 8: seven strips
POLY_DESC = 16            # ints per item row of tatt_poly_paste_u8 (include/tatt_hip.h)
POLY_STRIP_DESC = 32      # ints per strip row
# how the messages name a kind of region and what it takes: (prefix, a region, its points, the most points, the order of the points)
_QUAD = ("quads", "quad", "four (x, y) pairs of ints", POLY_MIN_POINTS, "top-left, top-right, bottom-right, bottom-left with y down")
_POLY = ("polys", "polygon", "an even number of (x, y) pairs of ints, %d to %d" % (POLY_MIN_POINTS, POLY_MAX_POINTS), POLY_MAX_POINTS,
         "top points in reading direction, then back along the bottom, with y down")

PolyMaps = namedtuple("PolyMaps", "rect paste bbox seams widths bh scale")
PolyPlan = namedtuple("PolyPlan", "arrays offsets warp resize desc lines upload nbytes out_floats polys")
PolyPastePlan = namedtuple("PolyPastePlan", "resize items strips layers order counts rects canvas_off pitch nbytes")


def poly_limits():
    """tatt_poly_limits: {'tile_h', 'tile_w', 'items', 'side', 'feather', 'desc', 'strip_desc', 'strips'} -- the tile of the paste kernel,
    the most items of one launch, the largest side of a line or a target, the largest feather, the ints per item row and per strip row,
    the most strips of one polygon.  A host-only entry: needs no GPU."""
    import ctypes
    from ._lib import LIB
    out = (ctypes.c_int * 8)()
    if LIB.tatt_poly_limits(out) != 0:
        raise RuntimeError("tatt_poly_limits failed")
    return dict(zip(("tile_h", "tile_w", "items", "side", "feather", "desc", "strip_desc", "strips"), (int(v) for v in out)))


def poly_strips(poly):
    """-> the N - 1 strips, strip k = (t_k, t_{k+1}, b_{k+1}, b_k): a quad in `quad_check`'s order"""
    n = len(poly) // 2
    return [(poly[k], poly[k + 1], poly[2 * n - 2 - k], poly[2 * n - 1 - k]) for k in range(n - 1)]


def poly_columns(poly):
    """-> (widths, starts): w_k columns of the crop for strip k, beginning at column U_k"""
    widths = [_r(max(_d2(p1, p0), _d2(p2, p3))) for p0, p1, p2, p3 in poly_strips(poly)]
    return widths, [sum(widths[:k]) for k in range(len(widths))]


def poly_size(poly):
    """-> (bw, bh), the size of the rectified crop: the strips' columns side by side, the longest seam rounded half up"""
    n = len(poly) // 2
    return sum(poly_columns(poly)[0]), max(_r(_d2(poly[s], poly[2 * n - 1 - s])) for s in range(n))


poly_bbox = quad_bbox     # -> (x0, y0, x1, y1), the bounding box of the points, however many


def _cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _interiors_overlap(p, q):
    """two strictly convex clockwise quads: whether their interiors meet (separating axes along the sides of both, in integers; quads
    that only touch do not overlap)"""
    for a, b in ((p, q), (q, p)):
        for i in range(4):
            if all(_cross(a[i], a[(i + 1) % 4], v) <= 0 for v in b):
                return False
    return True


def poly_check(size, polys, limits=None):
    """size = (Ws, Hs), polys: 2 N integer (x, y) points each, 2 <= N <= 8, the top of the text in reading direction then back along the
    bottom -> the polygons as a list of tuples of int pairs.  Every point in [0, Ws] x [0, Hs]; every strip strictly convex and clockwise
    with opposite sides within QUAD_MAX_TAPER of each other (exactly, on squared lengths) and at least 2 columns; bw and bh at least
    SCENE_MIN_SIDE; no two non-adjacent strips whose interiors overlap (the text may bend but not cross itself); at most
    scene_limits()['boxes'] polygons.  Anything else raises ValueError naming the polygon, and the strip where there is one."""
    return _check(size, polys, limits, _POLY)


def _check(size, regions, limits, kind):
    """`quad_check` (kind = _QUAD) and `poly_check` (_POLY): a quad is the polygon of four points, named whole where a polygon names
    its strip, and measured before its taper is looked at (the order of `quad_check`'s messages; the rules are the same: one strip of
    w_0 = bw >= SCENE_MIN_SIDE columns, and no second strip to cross)"""
    who, one, points, most, corners = kind
    lim = limits if limits is not None else scene_limits()
    ws, hs = int(size[0]), int(size[1])
    if ws < 1 or hs < 1 or ws > lim["side"] or hs > lim["side"]:
        raise ValueError("%s: the image is %d x %d; sides from 1 to %d are taken" % (who, ws, hs, lim["side"]))
    regions = list(regions)
    if len(regions) > lim["boxes"]:
        raise ValueError("%s: %d %ss; at most %d" % (who, len(regions), one, lim["boxes"]))
    out = []
    for k, region in enumerate(regions):
        try:
            ok = all(len(p) == 2 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in p) for p in region)
            count = len(region)
        except TypeError:
            ok, count = False, 0
        if not ok or count % 2 or not POLY_MIN_POINTS <= count <= most:
            raise ValueError("%s: %s %d must be %s; got %r" % (who, one, k, points, region))
        q = tuple((int(x), int(y)) for x, y in region)
        if not all(0 <= x <= ws and 0 <= y <= hs for x, y in q):
            raise ValueError("%s: %s %d = %s does not lie in the %d x %d image (0 <= x <= Ws, 0 <= y <= Hs)" % (who, one, k, q, ws, hs))
        strips = poly_strips(q)
        whole = most == POLY_MIN_POINTS
        name = lambda n: "%s %d = %s" % (one, k, q) if whole else "%s %d, strip %d = %s" % (one, k, n, strips[n])

        def sized():
            bw, bh = poly_size(q)
            if bw < SCENE_MIN_SIDE or bh < SCENE_MIN_SIDE:
                raise ValueError("%s: %s %d = %s rectifies to %d x %d; both sides must be at least SCENE_MIN_SIDE = %d" % (
                    who, one, k, q, bw, bh, SCENE_MIN_SIDE))

        def tapered(n):
            s = strips[n]
            for a, b in ((_d2(s[1], s[0]), _d2(s[2], s[3])), (_d2(s[3], s[0]), _d2(s[2], s[1]))):
                if max(a, b) > QUAD_MAX_TAPER ** 2 * min(a, b):
                    raise ValueError("%s: %s: opposite sides differ by more than QUAD_MAX_TAPER = %d" % (who, name(n), QUAD_MAX_TAPER))
        for n, s in enumerate(strips):
            if any(_cross(s[i], s[(i + 1) % 4], s[(i + 2) % 4]) <= 0 for i in range(4)):
                raise ValueError("%s: %s is not strictly convex and clockwise (%s)" % (who, name(n), corners))
            if not whole:
                tapered(n)
        if whole:                                                    # (its one strip has w_0 = bw >= SCENE_MIN_SIDE columns)
            sized()
            tapered(0)
        else:
            for n, w in enumerate(poly_columns(q)[0]):
                if w < 2:
                    raise ValueError("%s: %s takes %d column; at least 2" % (who, name(n), w))
            sized()
        for n in range(len(strips)):
            for m in range(n + 2, len(strips)):
                if _interiors_overlap(strips[n], strips[m]):
                    raise ValueError("%s: %s %d = %s crosses itself: strip %d and strip %d overlap" % (who, one, k, q, n, m))
        out.append(q)
    return out


# ---- the maps -------------------------------------------------------------------------------------------------------------------------
def poly_matrices(poly, scale: int = 1, rect: bool = True, paste: bool = True):
    """one checked polygon, the up-scaling factor -> PolyMaps(rect, paste, bbox, seams, widths, bh, scale).  rect[k]: nine ints, warps
    the scene into the (bh, w_k) columns [U_k, U_k + w_k) of the crop; paste[k]: nine ints, warps the strip's (scale bh, scale w_k) part
    of the line into the POLYGON's bounding box [scale bx0, scale bx1) x [scale by0, scale by1) of the up-scaled canvas (normalised at
    the strip's centroid; its gx is local to the strip); bbox = (bx0, by0, bx1, by1); seams[s - 1] = (A, B, C) of E_s for the interior
    seams s = 1 .. N - 2; widths = the w_k.  For N = 2 rect[0] and paste[0] are `quad_matrices`'s.  ValueError when the integers do not
    fit."""
    return _maps(poly, scale, rect, paste, _POLY)


def _maps(poly, scale, rect, paste, kind):
    """`poly_matrices`, and `quad_matrices` for the polygon of four points (kind = _QUAD: its one strip is named as the quad)"""
    poly = tuple((int(x), int(y)) for x, y in poly)
    _scale_check(kind[0], scale)
    n = len(poly) // 2
    widths, _ = poly_columns(poly)
    bh = poly_size(poly)[1]
    bx0, by0, bx1, by1 = poly_bbox(poly)
    s = scale
    half = _diag(Fraction(1, 2), Fraction(1, 2))
    shift = [[Fraction(1), 0, Fraction(s * bx0)], [0, Fraction(1), Fraction(s * by0)], [0, 0, Fraction(1)]]
    tail = _mul(_mul(_diag(Fraction(1, s), Fraction(1, s)), shift), half)
    rects, pastes = [] if rect else None, [] if paste else None
    for k, strip in enumerate(poly_strips(poly)):
        what = "quad %s" % (poly,) if kind is _QUAD else "polygon %s, strip %d" % (poly, k)
        hf = _homography(strip, widths[k], bh)
        if rect:
            rects.append(_integer(_mul(hf, half), widths[k], bh, bh, widths[k], True, what))
        if paste:
            q = _mul(_mul(_diag(s, s), _adjugate(hf)), tail)
            mx, my = Fraction(sum(p[0] for p in strip), 4), Fraction(sum(p[1] for p in strip), 4)
            pastes.append(_integer(q, 2 * s * (mx - bx0), 2 * s * (my - by0), s * (by1 - by0), s * (bx1 - bx0), False, what))
    seams = []
    for i in range(1, n - 1):
        (tx, ty), (ux, uy) = poly[i], poly[2 * n - 1 - i]
        dx, dy = ux - tx, uy - ty
        seams.append((dy, -dx, 2 * s * (dx * (ty - by0) - dy * (tx - bx0))))
    return PolyMaps(rects, pastes, (bx0, by0, bx1, by1), seams, widths, bh, s)


def _rectify(a, strips, bh):
    """the (bh, bw, 3) crop of the (matrix, width) strips of a region, side by side"""
    import numpy as np
    return np.concatenate([warp_u8_host(a, m, bh, w) for m, w in strips], axis=1)


def _rect_strips(poly):
    """one checked polygon -> the (m_rect, w_k) of its strips"""
    maps = poly_matrices(poly, 1, paste=False)
    return list(zip(maps.rect, maps.widths))


def poly_rectify_host(scene, poly):
    """RGB PIL image (or an (Hs, Ws, 3) uint8 array), one checked polygon -> the (bh, bw, 3) uint8 rectified crop"""
    import numpy as np
    return _rectify(np.asarray(scene), _rect_strips(poly), poly_size(poly)[1])


def _strip_claims(maps, out_h, out_w, H):
    """-> per strip (claim mask, gx, gy): what the strip claims on its own, before 'the first strip wins'"""
    import numpy as np
    J = 2 * np.arange(out_w, dtype=np.int64)[None, :] + 1
    I = 2 * np.arange(out_h, dtype=np.int64)[:, None] + 1
    with np.errstate(over="ignore"):
        E = [np.int64(a) * J + np.int64(b) * I + np.int64(c) for a, b, c in maps.seams]
    last, res = len(maps.paste) - 1, []
    for k, m in enumerate(maps.paste):
        gx, gy, ok = _warp_coords(m, out_h, out_w)
        ok = ok & (gy >= 0) & (gy < 256 * H)
        if k >= 1:
            ok &= E[k - 1] >= 0
        if k < last:
            ok &= E[k] < 0
        if k == 0:
            ok &= gx >= 0
        if k == last:
            ok &= gx < 256 * maps.scale * maps.widths[k]
        res.append((ok, gx, gy))
    return res


def poly_owner_host(maps, out_h=None, out_w=None, strips=None):
    """-> the (out_h, out_w) int array of the strip that paints each pixel of the bounding box (the box's own size by default), -1 where
    none does; strips: only these strips are tried"""
    import numpy as np
    x0, y0, x1, y1 = maps.bbox
    out_h = maps.scale * (y1 - y0) if out_h is None else out_h
    out_w = maps.scale * (x1 - x0) if out_w is None else out_w
    owner = np.full((out_h, out_w), -1, np.int64)
    for k, (ok, _, _) in enumerate(_strip_claims(maps, out_h, out_w, maps.scale * maps.bh)):
        if strips is None or k in strips:
            owner[ok & (owner < 0)] = k
    return owner


def poly_paste_host(line, maps, dst, feather=None, strips=None):
    """line: the (scale bh, scale bw, 3) uint8 finished line, maps: `poly_matrices(poly, scale)`, dst: an (OH, OW, 3) uint8 array, the
    polygon's bounding box of the canvas (any OH, OW >= 1: pixels beyond the box are judged like all others) -> dst, painted in place by
    the rule of the module's docstring with feather F (None = 0).  strips: only these strips are tried (the others paint nothing)."""
    import numpy as np
    line = np.asarray(line)
    H, W = maps.scale * maps.bh, maps.scale * sum(maps.widths)
    if line.shape != (H, W, 3) or line.dtype != np.uint8:
        raise ValueError("poly_paste_host takes the (%d, %d, 3) uint8 line; got %s %s" % (H, W, line.shape, line.dtype))
    F = 0 if feather is None else int(feather)
    if F < 0 or dst.ndim != 3 or dst.shape[2] != 3 or dst.dtype != np.uint8 or dst.shape[0] < 1 or dst.shape[1] < 1:
        raise ValueError("poly_paste_host: dst must be (OH, OW, 3) uint8 and the feather >= 0")
    out_h, out_w = dst.shape[:2]
    old = dst.astype(np.int64)
    done = np.zeros((out_h, out_w), bool)
    start = 0
    for k, (ok, gx, gy) in enumerate(_strip_claims(maps, out_h, out_w, H)):
        with np.errstate(over="ignore"):
            gxg = gx + np.int64(256 * maps.scale * start)
        start += maps.widths[k]
        if strips is not None and k not in strips:
            continue
        ok = ok & ~done
        done |= ok
        dst[ok] = _sample_host(line, gxg, gy, F, old)[ok].astype(np.uint8)
    return dst


# ---- the composition ------------------------------------------------------------------------------------------------------------------
def poly_windows_host(scene, polys, lr_size=(16, 64), stride: int = 32, mask: bool = True):
    """RGB PIL image, polygons -> (stack, lines): the concatenation of `line_windows_host(rectified crop, ...)` over the polygons, an
    (n_windows, 3 + mask, h, w) float stack, and lines[k] = Line(wl, starts, first window index) of polygon k."""
    import numpy as np
    from PIL import Image
    a = np.asarray(scene)
    return _region_windows_host(poly_check(scene.size, polys), lambda poly: Image.fromarray(poly_rectify_host(a, poly), "RGB"), lr_size,
                                stride, mask)


def poly_layers(polys):
    """`scene_layers` on the polygons' bounding boxes: pastes of one layer have disjoint destination rectangles"""
    return scene_layers([poly_bbox(p) for p in polys])


def poly_compose_host(scene, polys, line_images, scale: int, feather: int = 0, order=None):
    """-> the RGB PIL image of size (scale * Ws, scale * Hs): the canvas is `scene.resize((scale * Ws, scale * Hs), BICUBIC)`; polygon
    k's line image (RGB PIL, or an (H, W, 3) uint8 array) is resized with PIL bicubic to (scale * bw, scale * bh) and pasted
    (`poly_paste_host`) into the polygon's bounding box of the canvas, in input order (`order`: another order of the indices, e.g. layer
    after layer).  feather = F >= 0; a polygon of four points gets the bytes `quad_compose_host` gives its quad."""
    from PIL import Image
    polys = poly_check(scene.size, polys)
    _scale_check("polys", scale)
    canvas, line = _compose_front(("polys", "polygons"), scene, len(polys), line_images, scale, feather)
    for k in (range(len(polys)) if order is None else order):
        bw, bh = poly_size(polys[k])
        maps = poly_matrices(polys[k], scale, rect=False)
        x0, y0, x1, y1 = maps.bbox
        poly_paste_host(line(k, scale * bw, scale * bh), maps, canvas[scale * y0:scale * y1, scale * x0:scale * x1], feather)
    return Image.fromarray(canvas, "RGB")


def super_resolve_polys_host(scene, polys, run_windows, lr_size=(16, 64), stride: int = 32, mask: bool = True, rule: str = "floor",
                             c0: int = 0, feather: int = 0, scale=None):
    """The composition on the host: `poly_windows_host` -> per polygon `run_windows` (a callable: the (n, 3 + mask, h, w) windows of ONE
    polygon -> their (n, C, H, W) SR windows) -> `blend_windows_host` -> `poly_compose_host`.  The scale is H // h; `scale` must be given
    when there is no polygon to take it from (and is checked against the model's otherwise)."""
    return _super_resolve_boxes_host(poly_windows_host, poly_compose_host, ("polys", "polygons"), scene, polys, run_windows, lr_size,
                                     stride, mask, rule, c0, feather, scale)


# ---- host halves of the launches ------------------------------------------------------------------------------------------------------
def poly_item_row(src_off, hs, ws, sp, dst_off, oh, ow, dp, feather, first, count):
    """one POLY_DESC-int item row of tatt_poly_paste_u8: [line byte offset, H, W, line pitch, target byte offset, OH, OW, target pitch,
    feather, first strip row, strip count, 0 x 5]"""
    row = [src_off, hs, ws, sp, dst_off, oh, ow, dp, feather, first, count]
    return row + [0] * (POLY_DESC - len(row))


def poly_strip_row(start, width, m, enter=None, leave=None):
    """one POLY_STRIP_DESC-int strip row: [scale U_k, scale w_k, the nine entries of m_paste as (low, high) words, A, B, C of the seam
    the strip begins at (zeros for the first strip), A, B, C of the seam it ends at (zeros for the last strip), as (low, high) words]"""
    row = [start, width]
    for v in tuple(m) + tuple(enter or (0, 0, 0)) + tuple(leave or (0, 0, 0)):
        row += _words(v)
    return row


def poly_plan(scene, polys, lr_size=(16, 64), stride: int = 32, mask: bool = True, limits=None, slimits=None, qlimits=None):
    """Host half of `DeviceCollator.poly_windows`, without a device: `quad_plan` with one mode-0 tatt_warp_u8 row per STRIP -> PolyPlan(
    arrays, offsets, warp, resize, desc, lines, upload, nbytes, out_floats, polys), laid out as `quad_plan` lays it out.  Strip k of a
    polygon is warped into the crop's region at byte offset + 3 U_k with OW = w_k and the crop's pitch 3 bw: still ONE launch for all
    strips of all polygons.  An over-size crop goes the ways of `quad_plan`: resized on the device, or rectified and resized on the host
    and uploaded."""
    return PolyPlan(*_window_plan(scene, polys, lr_size, stride, mask, limits, slimits, qlimits, _POLY, _rect_strips))


def _resize_takes(hs, ws, oh, ow, slim):
    """what tatt_resize_u8 takes (`scene_limits`)"""
    return max(hs, ws, oh, ow) <= slim["side"] and hs <= slim["down"] * oh and ws <= slim["down"] * ow


def _window_plan(scene, regions, lr_size, stride, mask, limits, slimits, qlimits, kind, strips):
    """`quad_plan` (kind = _QUAD) and `poly_plan` (_POLY) -> the fields of their plans, the checked regions last.  strips(region): the
    (m_rect, width) of its strips, one mode-0 warp row each, side by side in the region's crop; a quad has one."""
    import numpy as np
    from PIL import Image
    lim = limits if limits is not None else line_limits()
    slim = slimits if slimits is not None else scene_limits()
    qlim = qlimits if qlimits is not None else quad_limits()
    if getattr(scene, "mode", None) != "RGB":
        raise ValueError("DeviceCollator takes RGB PIL images (Image.open(..).convert('RGB')); the scene is %r" % (
            getattr(scene, "mode", type(scene).__name__),))
    regions = _check(scene.size, regions, slim, kind)
    h, w = int(lr_size[0]), int(lr_size[1])
    if not (1 <= h <= lim["h"] and 1 <= w <= lim["w"]):
        raise ValueError("tatt_scene_windows takes windows up to %d x %d (got %d x %d)" % (lim["h"], lim["w"], h, w))
    a = np.asarray(scene)
    Hs, Ws = a.shape[:2]
    if max(Hs, Ws) > qlim["side"] or sum(len(p) // 2 - 1 for p in regions) > qlim["items"]:
        raise ValueError("tatt_warp_u8 takes sides up to %d and %d items" % (qlim["side"], qlim["items"]))
    geo = []
    for k, region in enumerate(regions):
        bw, bh = poly_size(region)
        wl, starts = line_plan((bw, bh), (h, w), stride)
        if wl > lim["wl"] or len(starts) > lim["windows"]:
            raise ValueError("tatt_scene_windows takes lines up to %d columns and %d windows (%s %d: %d, %d)" % (
                lim["wl"], lim["windows"], kind[1], k, wl, len(starts)))
        if max(bw, bh) > qlim["side"]:
            raise ValueError("tatt_warp_u8 takes crops up to %d a side (%s %d: %d x %d)" % (qlim["side"], kind[1], k, bw, bh))
        how = "crop" if _line_takes(bh, bw, h, wl, w, lim) else "device" if _resize_takes(bh, bw, h, wl, slim) else "host"
        geo.append((region, bw, bh, wl, starts, how))
    arrays, offsets, off = [a], [0], _up(a.size)
    src = {}
    for k, (region, bw, bh, wl, starts, how) in enumerate(geo):     # uploaded sources first: the upload is one contiguous copy
        if how == "host":
            small = np.asarray(Image.fromarray(_rectify(a, strips(region), bh), "RGB").resize((wl, h), Image.BICUBIC))
            arrays.append(small)
            offsets.append(off)
            src[k] = (off, h, wl, 3 * wl)
            off += _up(small.size)
    upload = off
    warp, resize = [], []
    for k, (region, bw, bh, wl, starts, how) in enumerate(geo):
        if how == "host":
            continue
        start = 0
        for m, wk in strips(region):                                 # one row per strip, side by side in the crop
            warp.append(warp_row(0, Hs, Ws, 3 * Ws, off + 3 * start, bh, wk, 3 * bw, 0, 0, m))
            start += wk
        crop = (off, bh, bw, 3 * bw)
        off += _up(bh * 3 * bw)
        if how == "device":
            resize.append([crop[0], bh, bw, 3 * bw, off, h, wl, 3 * wl, 0] + [0] * (RESIZE_DESC - 9))
            src[k] = (off, h, wl, 3 * wl)
            off += _up(h * 3 * wl)
        else:
            src[k] = crop
        if off >= 2 ** 31:
            raise ValueError("DeviceCollator: the scene does not fit 32-bit offsets")
    rows, lines, out_off, planes = [], [], 0, 3 + int(bool(mask))
    for k, (region, bw, bh, wl, starts, how) in enumerate(geo):
        o, sh, sw, sp = src[k]
        lines.append(Line(wl, starts, len(rows)))
        for x in starts:
            rows.append((o, sh, sw, h, wl, x, w, int(bool(mask)), out_off, sp, 0, 0, 0, 0, 0, 0))
            out_off += planes * h * w
    if off >= 2 ** 31 or out_off >= 2 ** 31:
        raise ValueError("DeviceCollator: the scene does not fit 32-bit offsets")
    return (arrays, offsets, np.array(warp, np.int32).reshape(-1, QUAD_DESC), np.array(resize, np.int32).reshape(-1, RESIZE_DESC),
            np.array(rows, np.int32).reshape(-1, SCENE_DESC), lines, upload, off, out_off, regions)


poly_fill = quad_fill     # a PolyPlan shares the QuadPlan's layout: warp rows | resize rows | window rows | sources


def poly_paste_plan(size, polys, blend_desc, blend_bytes, scale: int, H: int, feather: int = 0, limits=None, plimits=None):
    """Host half of `DeviceExporter.scene_polys`, without a device: `quad_paste_plan` with the rows of tatt_poly_paste_u8 in place of
    the mode-1 warp rows -> PolyPastePlan(resize, items, strips, layers, order, counts, rects, canvas_off, pitch, nbytes).  Behind the
    line canvases, 16-byte aligned: rects[k], the (scale * bh, scale * bw) line of polygon k (pitch 3 * scale * bw), then the canvas at
    canvas_off (pitch 3 * scale * Ws).  resize: (1 + n, RESIZE_DESC) rows of tatt_resize_u8: row 0 the background, rows 1 .. n in input
    order: line canvas -> rectangle (ONE launch).  items: (n, POLY_DESC) item rows in paste order `order` = by (layer, index), counts[l]
    polygons in layer l: one launch each; strips: (total strips, POLY_STRIP_DESC), the ONE strip table all launches share, the strips
    of an item consecutive from its 'first strip row'."""
    import numpy as np
    polys, maps, resize, rects, canvas_off, pitch, nbytes, layers, order, counts = _paste_front(
        size, polys, blend_desc, blend_bytes, scale, H, feather, limits, plimits if plimits is not None else poly_limits(), _POLY,
        lambda poly: poly_matrices(poly, scale, rect=False))
    items, strips = [], []
    for k in order:
        mp = maps[k]
        x0, y0, x1, y1 = mp.bbox
        bw = sum(mp.widths)
        items.append(poly_item_row(rects[k], scale * mp.bh, scale * bw, 3 * scale * bw, canvas_off + scale * y0 * pitch + 3 * scale * x0,
                                   scale * (y1 - y0), scale * (x1 - x0), pitch, feather, len(strips), len(mp.paste)))
        start, last = 0, len(mp.paste) - 1
        for n, m in enumerate(mp.paste):
            strips.append(poly_strip_row(scale * start, scale * mp.widths[n], m, mp.seams[n - 1] if n else None,
                                         mp.seams[n] if n < last else None))
            start += mp.widths[n]
    return PolyPastePlan(resize, np.array(items, np.int32).reshape(-1, POLY_DESC), np.array(strips, np.int32).reshape(-1, POLY_STRIP_DESC),
                         layers, order, counts, rects, canvas_off, pitch, nbytes)


def _paste_front(size, regions, blend_desc, blend_bytes, scale, H, feather, limits, klimits, kind, maps):
    """`quad_paste_plan` (kind = _QUAD, klimits = `quad_limits()`) and `poly_paste_plan` (_POLY, `poly_limits()`) in front of the rows
    of their own paste launches -> (the checked regions, maps(region) of each, resize, rects, canvas_off, pitch, nbytes, layers, order,
    counts) as both plans state them"""
    import numpy as np
    who, one = kind[:2]
    lim = limits if limits is not None else scene_limits()
    regions = _check(size, regions, lim, kind)
    ws, hs = int(size[0]), int(size[1])
    side, fmax = min(lim["side"], klimits["side"]), min(lim["feather"], klimits["feather"])
    _scale_check(who, scale)
    if not (isinstance(feather, int) and not isinstance(feather, bool) and 0 <= feather <= fmax):
        raise ValueError("%s: feather must be an int in [0, %d]; got %r" % (who, fmax, feather))
    if len(blend_desc) != len(regions):
        raise ValueError("%s: %d lines for %d %ss" % (who, len(blend_desc), len(regions), one))
    if scale * max(ws, hs) > side:
        raise ValueError("%s: the canvas %d x %d is beyond the largest side %d" % (who, scale * ws, scale * hs, side))
    if "strips" in klimits and (len(regions) > klimits["items"] or any(len(p) // 2 - 1 > klimits["strips"] for p in regions)):
        raise ValueError("tatt_poly_paste_u8 takes %d items of up to %d strips" % (klimits["items"], klimits["strips"]))
    off = _up(blend_bytes)
    resize = np.zeros((1 + len(regions), RESIZE_DESC), np.int32)
    rects, mats = [], []
    for k, region in enumerate(regions):
        bw, bh = poly_size(region)
        d = blend_desc[k]
        lw = int(d[3]) * int(d[2])                                   # scale * wl columns of the line canvas
        oh, ow = scale * bh, scale * bw
        if H > lim["down"] * oh or lw > lim["down"] * ow or max(oh, ow) > side:
            raise ValueError("%s: %s %d: resizing %d x %d into %d x %d is beyond the limits" % (who, one, k, H, lw, oh, ow))
        resize[1 + k, :9] = (int(d[6]), H, lw, int(d[7]), off, oh, ow, 3 * ow, 0)
        rects.append(off)
        mats.append(maps(region))
        off += _up(oh * 3 * ow)
        if off >= 2 ** 31:
            raise ValueError("DeviceExporter: the scene does not fit 32-bit offsets")
    canvas_off, pitch = off, 3 * scale * ws
    nbytes = canvas_off + scale * hs * pitch
    if nbytes >= 2 ** 31 or hs * ws * 3 >= 2 ** 31:
        raise ValueError("DeviceExporter: the scene does not fit 32-bit offsets")
    resize[0, :9] = (0, hs, ws, 3 * ws, canvas_off, scale * hs, scale * ws, pitch, 0)
    return (regions, mats, resize, rects, canvas_off, pitch, nbytes) + _paste_order([poly_bbox(p) for p in regions])
