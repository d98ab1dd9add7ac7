"""Where in the picture a span of a read line lies: the geometry that carries the columns of a `read.CharSpan` or a `read.WordSpan` back
through the map that made the line (`infer.SuperResolver(read_locate=True)`, `PendingScene.locations()`, `PendingUpscale.locations()`).

A region (a box of `scene`, a quad of `scene_quads`, a polygon of `scene_polys`) is straightened into a crop of bw x bh pixels, the crop
is super-resolved into a line canvas of width W, and the reader states its spans in columns [x0, x1) of that canvas.  Stated in
`fractions.Fraction`, converted to float once at the end:
* the column x of the canvas is the crop abscissa u = x bw / W;
* a box (bx0, by0, bx1, by1) gives the rectangle scale (bx0 + x (bx1 - bx0) / W) by scale by0 .. scale by1;
* a quad gives `quads._homography(quad, bw, bh)` -- the exact rational map its integer matrices are derived from -- at (u, 0) and
  (u, bh), times scale;
* a polygon uses the strip k with U_k <= u <= U_k + w_k (the LOWER strip on a seam; either gives the same point) and that strip's
  rational map at (u - U_k, v).  A span that crosses interior seams takes the seams' own vertices t_s, b_s (times scale) into its
  outline, so the outline follows the polygon;
* a line of `long_lines` gives the rectangle in the returned image, scaled by its `out_sizes` entry where there is one.
An outline is in the polygon convention of `polys.py`: the top points in reading direction, then the bottom points back -- clockwise with
y down.  Nothing here touches a device; the pixels that were painted are the integer plans' (`quads.quad_matrices`,
`polys.poly_matrices`), which round these maps: an outline says where a span lies, to within that rounding."""
from __future__ import annotations

import numbers
from collections import namedtuple
from fractions import Fraction

from .polys import poly_columns, poly_size, poly_strips
from .quads import _homography, quad_size
from .read import CharSpan

LocatedChar = namedtuple("LocatedChar", CharSpan._fields + ("polygon",))


def region_kind(region) -> str:
    """'box' for four integers, 'quad' for four points, 'poly' for 2 N >= 6 points; ValueError for anything else"""
    try:
        if len(region) == 4 and all(isinstance(v, numbers.Integral) for v in region):
            return "box"
        if len(region) >= 4 and len(region) % 2 == 0 and all(len(p) == 2 and all(isinstance(v, numbers.Integral) for v in p)
                                                             for p in region):
            return "quad" if len(region) == 4 else "poly"
    except TypeError:
        pass
    raise ValueError("locate: a region is a box (x0, y0, x1, y1), a quad of four (x, y) points or a polygon of 2 N points, in ints; "
                     "got %r" % (region,))


def _project(h, u, v):
    """the rational map h at (u, v) -> (X, Y)"""
    X, Y, Wd = (h[r][0] * u + h[r][1] * v + h[r][2] for r in range(3))
    return X / Wd, Y / Wd


def _check_span(W, x0, x1):
    if not all(isinstance(v, (numbers.Integral, Fraction)) for v in (W, x0, x1)) or not (W >= 1 and 0 <= x0 <= x1 <= W):
        raise ValueError("locate: a span is 0 <= x0 <= x1 <= W in ints or Fractions; got x0 = %r, x1 = %r, W = %r" % (x0, x1, W))


def region_size(region):
    """-> (bw, bh) of the region's straightened crop"""
    kind = region_kind(region)
    if kind == "box":
        return region[2] - region[0], region[3] - region[1]
    return quad_size(region) if kind == "quad" else poly_size(region)


def poly_point(poly, u, v):
    """the point of the polygon that the crop point (u, v) stands for, 0 <= u <= bw, as Fractions (scale 1): strip k with
    U_k <= u <= U_k + w_k, the lower strip on a seam"""
    widths, starts = poly_columns(poly)
    bh = poly_size(poly)[1]
    k = next((k for k in range(len(widths)) if u <= starts[k] + widths[k]), len(widths) - 1)
    return _project(_homography(poly_strips(poly)[k], widths[k], bh), u - starts[k], v)


def span_polygon_exact(region, W, x0, x1, scale=1):
    """`span_polygon` in Fractions: [(X, Y)]"""
    _check_span(W, x0, x1)
    kind, s = region_kind(region), Fraction(scale)
    bw, bh = region_size(region)
    u0, u1 = Fraction(x0 * bw, W), Fraction(x1 * bw, W)
    if kind == "box":
        bx0, by0, bx1, by1 = region
        return [(s * (bx0 + u0), s * by0), (s * (bx0 + u1), s * by0), (s * (bx0 + u1), s * by1), (s * (bx0 + u0), s * by1)]
    if kind == "quad":
        h = _homography(tuple(tuple(p) for p in region), bw, bh)
        pts = [_project(h, u0, 0), _project(h, u1, 0), _project(h, u1, bh), _project(h, u0, bh)]
        return [(s * x, s * y) for x, y in pts]
    poly = tuple(tuple(p) for p in region)
    n = len(poly) // 2
    _, starts = poly_columns(poly)
    inner = [k for k in range(1, n - 1) if u0 < starts[k] < u1]      # the interior seams the span crosses
    top = [poly_point(poly, u0, 0)] + [poly[k] for k in inner] + [poly_point(poly, u1, 0)]
    bottom = [poly_point(poly, u1, bh)] + [poly[2 * n - 1 - k] for k in reversed(inner)] + [poly_point(poly, u0, bh)]
    return [(s * x, s * y) for x, y in top + bottom]


def span_polygon(region, W, x0, x1, scale=1):
    """The outline, in the up-scaled picture, of the columns [x0, x1) of the line canvas of width W that was read for `region` (a box
    (x0, y0, x1, y1) of `scene`, a quad of `scene_quads`, a polygon of `scene_polys`; scale: the SR factor) -> [(x, y)] floats, the top
    points in reading direction, then the bottom points back.  Serves a `read.CharSpan` and a `read.WordSpan` alike."""
    return [(float(x), float(y)) for x, y in span_polygon_exact(region, W, x0, x1, scale)]


def line_polygon_exact(H, W, x0, x1, out_size=None):
    """`line_polygon` in Fractions"""
    _check_span(W, x0, x1)
    ow, oh = (W, H) if out_size is None else (int(out_size[0]), int(out_size[1]))
    a, b = Fraction(x0 * ow, W), Fraction(x1 * ow, W)
    return [(a, Fraction(0)), (b, Fraction(0)), (b, Fraction(oh)), (a, Fraction(oh))]


def line_polygon(H, W, x0, x1, out_size=None):
    """The rectangle, in the image a `long_lines` call returns for a line (its (H, W) canvas, or that canvas resized to
    out_size = (width, height)), of the columns [x0, x1) of the canvas -> [(x, y)] floats"""
    return [(float(x), float(y)) for x, y in line_polygon_exact(H, W, x0, x1, out_size)]


def located(location, outline):
    """a `read.LineLocation` with every character as a `LocatedChar`: outline(x0, x1) -> the character's polygon"""
    return location._replace(chars=[LocatedChar(*c, outline(c.x0, c.x1)) for c in location.chars])


def locate_regions(locations, regions, widths, scale):
    """the LineLocations of the lines read for `regions` (canvas widths `widths`) with their characters' polygons in the picture"""
    return [located(loc, lambda x0, x1, r=r, W=W: span_polygon(r, int(W), x0, x1, scale)) for loc, r, W in zip(locations, regions, widths)]


def locate_lines(locations, sizes, out_sizes=None):
    """the LineLocations of `long_lines` images (canvas sizes (H, W)) with their characters' rectangles in the returned images"""
    outs = [None] * len(locations) if out_sizes is None else list(out_sizes)
    return [located(loc, lambda x0, x1, H=H, W=W, o=o: line_polygon(int(H), int(W), x0, x1, o)) for loc, (H, W), o in zip(locations, sizes, outs)]
