"""The geometry of tatt_amd/locate.py in exact Fractions: the span [0, W) is the region itself, an axis-aligned quad is its box, a polygon
of four points its quad, adjacent spans share their common edge, a seam point is the same from either strip, outlines are clockwise."""
from fractions import Fraction

import pytest

BOX = (7, 5, 71, 23)
QUAD = ((10, 12), (120, 4), (126, 40), (14, 52))
POLYS = (((10, 30), (60, 14), (110, 12), (160, 28), (156, 58), (110, 44), (60, 46), (16, 60)),          # N = 4: an arch, three strips
         ((4, 8), (50, 8), (96, 20), (92, 50), (50, 38), (4, 38)),                                      # N = 3
         ((20, 10), (90, 16), (88, 44), (18, 40)))                                                      # N = 2: a quad
W, SCALE = 200, 2


def area2(pts):
    """twice the signed area: positive = clockwise with y down"""
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(pts, pts[1:] + pts[:1]))


def test_the_whole_line_is_the_region_itself():
    from tatt_amd import locate
    got = locate.span_polygon_exact(BOX, W, 0, W, SCALE)
    assert got == [(14, 10), (142, 10), (142, 46), (14, 46)] and all(isinstance(v, Fraction) for p in got for v in p)
    assert locate.span_polygon_exact(QUAD, W, 0, W, SCALE) == [(SCALE * x, SCALE * y) for x, y in QUAD]
    for poly in POLYS:                                               # every vertex of the chain, in the polygon's own order
        assert locate.span_polygon_exact(poly, W, 0, W, SCALE) == [(SCALE * x, SCALE * y) for x, y in poly], poly
    assert locate.span_polygon(BOX, W, 0, W, SCALE) == [(14.0, 10.0), (142.0, 10.0), (142.0, 46.0), (14.0, 46.0)]
    assert all(isinstance(v, float) for p in locate.span_polygon(QUAD, W, 3, 50, SCALE) for v in p)


def test_an_axis_aligned_quad_is_its_box_and_four_points_are_a_quad():
    from tatt_amd import locate
    x0, y0, x1, y1 = BOX
    as_quad = ((x0, y0), (x1, y0), (x1, y1), (x0, y1))
    assert locate.region_size(as_quad) == locate.region_size(BOX) == (64, 18)
    for a, b in ((0, W), (0, 1), (13, 57), (199, 200), (40, 40)):
        assert locate.span_polygon_exact(as_quad, W, a, b, SCALE) == locate.span_polygon_exact(BOX, W, a, b, SCALE)
        assert locate.span_polygon_exact(POLYS[2], W, a, b, 3) == locate.span_polygon_exact(tuple(POLYS[2]), W, a, b, 3)
        assert locate.region_kind(POLYS[2]) == "quad"
    # the N = 2 chain through the polygon's own code path equals the quad's
    poly = POLYS[2]
    for u in (0, Fraction(7, 3), 35, locate.region_size(poly)[0]):
        for v in (0, locate.region_size(poly)[1]):
            from tatt_amd.quads import _homography, quad_size
            assert locate.poly_point(poly, Fraction(u), v) == locate._project(_homography(poly, *quad_size(poly)), Fraction(u), v)


def test_adjacent_spans_share_their_edge_and_outlines_are_clockwise():
    from tatt_amd import locate
    cuts = [0, 9, 10, 47, 81, 100, 133, 160, 199, 200]
    for region in (BOX, QUAD) + POLYS:
        for a, b, c in zip(cuts, cuts[1:], cuts[2:]):
            left, right = locate.span_polygon_exact(region, W, a, b, SCALE), locate.span_polygon_exact(region, W, b, c, SCALE)
            n, m = len(left) // 2, len(right) // 2
            assert left[n - 1] == right[0] and left[n] == right[-1], (region, a, b, c)       # top and bottom of the common edge
            assert area2(left) > 0 and area2(right) > 0 and len(left) % 2 == 0
        assert area2(locate.span_polygon_exact(region, W, 0, W, SCALE)) > 0


def test_a_seam_point_is_the_same_from_either_strip_and_a_span_takes_the_seams_it_crosses():
    from tatt_amd import locate
    from tatt_amd.polys import poly_columns, poly_size, poly_strips
    from tatt_amd.quads import _homography
    for poly in POLYS[:2]:
        n = len(poly) // 2
        widths, starts = poly_columns(poly)
        bw, bh = poly_size(poly)
        strips = poly_strips(poly)
        for s in range(1, n - 1):
            lower = _homography(strips[s - 1], widths[s - 1], bh)
            upper = _homography(strips[s], widths[s], bh)
            # (at the seam's two ends, the points an outline takes; BETWEEN them two projective maps run along the seam at their own pace)
            for v, vertex in ((0, poly[s]), (bh, poly[2 * n - 1 - s])):
                a, b = locate._project(lower, Fraction(widths[s - 1]), v), locate._project(upper, Fraction(0), v)
                assert a == b == locate.poly_point(poly, Fraction(starts[s]), v) == vertex
        # a span from inside strip 0 to inside the last strip: every interior seam's vertices, top forward and bottom back
        Wc = 4 * bw
        got = locate.span_polygon_exact(poly, Wc, 4, Wc - 4, 3)
        assert len(got) == 2 * n and got[1:n - 1] == [(3 * x, 3 * y) for x, y in poly[1:n - 1]]
        assert got[n + 1:2 * n - 1] == [(3 * x, 3 * y) for x, y in poly[n + 1:2 * n - 1]]
        # a span that ENDS on a seam does not repeat the seam's vertex
        assert len(locate.span_polygon_exact(poly, Wc, 4, 4 * starts[1], 3)) == 4
        assert len(locate.span_polygon_exact(poly, Wc, 4 * starts[1], 4 * starts[1] + 4, 3)) == 4


def test_lines_and_the_characters_polygons():
    from tatt_amd import locate, read
    assert locate.line_polygon_exact(32, 128, 16, 48) == [(16, 0), (48, 0), (48, 32), (16, 32)]
    assert locate.line_polygon_exact(32, 128, 16, 48, (64, 20)) == [(8, 0), (24, 0), (24, 20), (8, 20)]
    assert locate.line_polygon(32, 100, 1, 2, (33, 7)) == [(0.33, 0.0), (0.66, 0.0), (0.66, 7.0), (0.33, 7.0)]
    loc = read.LineLocation("ab", -1.0, [read.CharSpan("a", 1, 0, 1, 0, 8, -0.25), read.CharSpan("b", 2, 3, 3, 13, 19, -0.5)], 100, False, 0)
    got = locate.locate_regions([loc, loc], [BOX, POLYS[1]], [100, 64], 2)
    assert [g._replace(chars=None) for g in got] == [loc._replace(chars=None)] * 2
    for g, region, Wl in zip(got, (BOX, POLYS[1]), (100, 64)):
        for c, want in zip(g.chars, loc.chars):
            assert isinstance(c, locate.LocatedChar) and c[:7] == tuple(want)
            assert c.polygon == locate.span_polygon(region, Wl, want.x0, want.x1, 2)
    lines = locate.locate_lines([loc], [(32, 100)], [(50, 16)])
    assert lines[0].chars[1].polygon == locate.line_polygon(32, 100, 13, 19, (50, 16))
    assert locate.locate_lines([loc], [(32, 100)])[0].chars[0].polygon == [(0.0, 0.0), (8.0, 0.0), (8.0, 32.0), (0.0, 32.0)]


def test_refusals():
    from tatt_amd import locate
    for region in ((1, 2, 3), ((1, 2), (3, 4), (5, 6)), (1.0, 2, 3, 4), "abcd", None, ((1, 2), (3, 4), (5, 6), (7,))):
        with pytest.raises(ValueError):
            locate.region_kind(region)
    for a, b in ((-1, 4), (5, 4), (0, 201), (0.5, 3)):
        with pytest.raises(ValueError):
            locate.span_polygon(BOX, W, a, b, 2)
