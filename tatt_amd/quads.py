"""Scene images with QUADRILATERAL text boxes (csrc/quads.hip; `DeviceCollator.quad_windows`, `DeviceExporter.scene_quads`,
`infer.SuperResolver.scene_quads`).

Scene-text detectors give four corner points per text instance, rotated and under perspective.  A quad is rectified into an upright
crop (a projective warp with a two-tap sampler per axis), the crop is a text line like a box of `tatt_amd/scene.py`, and the finished
line is warped back into the quad's place on the up-scaled picture: only the pixels of the quad are painted.

This module is the specification on the host, pure Python / numpy / PIL, and the yardstick of the kernel: the matrices are derived in
`fractions.Fraction` and rounded to integers ONCE, by the plan that both paths share; every pixel is 64-bit integer arithmetic with floor
division, so the device path equals it byte for byte.
* `quad_check` / `quad_size` / `quad_bbox`: what a list of quads must satisfy, the rectified size, the bounding box.
* `quad_matrices`: the two integer matrices (rectify, paste) of a quad.
* `warp_u8_host`: the warp itself, per destination pixel.
* `quad_rectify_host` / `quad_windows_host`: the crop and the window stack of all quads (`line_windows_host` of every crop).
* `quad_compose_host` / `super_resolve_quads_host`: the up-scaled scene with the SR lines warped in; the composition.
* `quad_limits` / `quad_plan` / `quad_fill` / `quad_paste_plan`: the host halves of the launches (tatt_warp_u8, tatt_resize_u8,
  tatt_scene_windows).

A quad is the polygon of four points of `tatt_amd/polys.py`, and everything that is not projective arithmetic has ONE body there: the
check, the matrices of a strip, the window plan, the front of the paste plan.  The `quad_*` functions below are entries onto those
bodies under the quad's own names and wording (they import from `polys` when called: `polys` imports this module).

A warp is stated per destination pixel (i, j) through a 3 x 3 integer matrix m applied to (J, I, 1), J = 2 j + 1, I = 2 i + 1 (the pixel
centre in half-pixel units):
    X = m00 J + m01 I + m02;   Y = m10 J + m11 I + m12;   Wd = m20 J + m21 I + m22                     (int64)
    gx = floor(256 X / Wd),    gy = floor(256 Y / Wd)             (Wd <= 0: the pixel is outside)
    fx = gx - 128, x0 = fx >> 8, ax = fx & 255;  fy, y0, ay alike
    v = ((256 - ay) ((256 - ax) p[y0][x0] + ax p[y0][x0 + 1]) + ay ((256 - ax) p[y0 + 1][x0] + ax p[y0 + 1][x0 + 1]) + 32768) >> 16
with the tap indices clamped to the source (border replicate).  Mode 0 (rectify) writes every destination pixel (zero where Wd <= 0, which
the plan excludes); mode 1 (paste) paints a pixel iff Wd > 0, 0 <= gx < 256 W_src and 0 <= gy < 256 H_src, feathered by its distance to
the nearest side of the SOURCE rectangle, and leaves every other pixel as it is.
"""
from __future__ import annotations

import math
from collections import namedtuple
from fractions import Fraction

from .lines import _compose_front, _region_windows_host, _scale_check, _super_resolve_boxes_host
from .scene import _up, scene_layers

QUAD_MAX_TAPER = 2        # opposite sides of a quad differ in length by at most this factor (a two-tap sampler aliases beyond it)
QUAD_SHIFT = 36           # fraction bits of the integer matrices
QUAD_DESC = 32            # ints per item row of tatt_warp_u8 (include/tatt_hip.h)
_BOUND = 1 << 62

QuadPlan = namedtuple("QuadPlan", "arrays offsets warp resize desc lines upload nbytes out_floats quads")
QuadPastePlan = namedtuple("QuadPastePlan", "resize warp layers order counts rects canvas_off pitch nbytes")


def quad_limits():
    """tatt_quad_limits: {'tile_h', 'tile_w', 'items', 'side', 'feather', 'desc'} -- the tile of the warp kernel, the most items of one
    launch, the largest side of a source or a target, the largest feather, the ints per descriptor row.  A host-only entry: needs no GPU."""
    import ctypes
    from ._lib import LIB
    out = (ctypes.c_int * 6)()
    if LIB.tatt_quad_limits(out) != 0:
        raise RuntimeError("tatt_quad_limits failed")
    return dict(zip(("tile_h", "tile_w", "items", "side", "feather", "desc"), (int(v) for v in out)))


def _r(n):
    """the square root of n rounded half up, in integers"""
    return (math.isqrt(4 * n) + 1) // 2


def _d2(a, b):
    return (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2


def quad_size(quad):
    """-> (bw, bh), the size of the rectified crop: the longer of the two opposite sides per direction, rounded half up"""
    p0, p1, p2, p3 = quad
    return _r(max(_d2(p1, p0), _d2(p2, p3))), _r(max(_d2(p3, p0), _d2(p2, p1)))


def quad_bbox(quad):
    """-> (x0, y0, x1, y1), the bounding box of the four points"""
    xs, ys = [p[0] for p in quad], [p[1] for p in quad]
    return min(xs), min(ys), max(xs), max(ys)


def quad_check(size, quads, limits=None):
    """size = (Ws, Hs), quads: ((x0, y0), (x1, y1), (x2, y2), (x3, y3)) integer points, the text's top-left, top-right, bottom-right and
    bottom-left corner (clockwise with y down, reading direction p0 -> p1) -> the quads as a list of tuples of int pairs.  Every point in
    [0, Ws] x [0, Hs], strictly convex and clockwise, both rectified sides at least SCENE_MIN_SIDE, opposite sides within QUAD_MAX_TAPER
    of each other (exactly, on squared lengths), at most scene_limits()['boxes'] quads; anything else raises ValueError naming the quad."""
    from .polys import _QUAD, _check
    return _check(size, quads, limits, _QUAD)


# ---- the matrices ---------------------------------------------------------------------------------------------------------------------
def _homography(quad, bw, bh):
    """the exact rational map of the rectangle [0, bw] x [0, bh] onto the quad: (0, 0) -> p0, (bw, 0) -> p1, (bw, bh) -> p2, (0, bh) -> p3
    (the closed form of the unit square's map, columns scaled by 1 / bw and 1 / bh)"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = quad
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dx2 * dy1
    if den == 0:
        raise ValueError("quads: %s is degenerate" % (quad,))
    g, h = Fraction(sx * dy2 - dx2 * sy, den), Fraction(dx1 * sy - sx * dy1, den)
    a, b, d, e = x1 - x0 + g * x1, x3 - x0 + h * x3, y1 - y0 + g * y1, y3 - y0 + h * y3
    return [[a / bw, b / bh, Fraction(x0)], [d / bw, e / bh, Fraction(y0)], [g / bw, h / bh, Fraction(1)]]


def _mul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _diag(x, y):
    return [[Fraction(x), 0, 0], [0, Fraction(y), 0], [0, 0, Fraction(1)]]


def _adjugate(m):
    """a multiple of the inverse (the normalisation by Wc fixes scale and sign)"""
    (a, b, c), (d, e, f), (g, h, i) = m
    return [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
            [d * h - e * g, b * g - a * h, a * e - b * d]]


def _integer(q, jc, ic, oh, ow, positive, what):
    """the rational matrix q -> nine ints m_ab = floor(q_ab 2^QUAD_SHIFT / Wc + 1 / 2), Wc = q's third row at (J, I) = (jc, ic); checked
    at the four corner pixels of the oh x ow destination (X, Y, Wd are linear: the corners bound every pixel)"""
    wc = q[2][0] * jc + q[2][1] * ic + q[2][2]
    if wc == 0:
        raise ValueError("quads: %s: the map is singular at its centre" % what)
    m = tuple(math.floor(v * (1 << QUAD_SHIFT) / wc + Fraction(1, 2)) for row in q for v in row)
    if any(abs(v) >= _BOUND for v in m):
        raise ValueError("quads: %s: the integer matrix does not fit 62 bits" % what)
    for J in (1, 2 * ow - 1):
        for I in (1, 2 * oh - 1):
            X, Y, Wd = (m[3 * r] * J + m[3 * r + 1] * I + m[3 * r + 2] for r in range(3))
            if abs(256 * X) >= _BOUND or abs(256 * Y) >= _BOUND or abs(Wd) >= _BOUND:
                raise ValueError("quads: %s: the warp does not fit 62 bits at pixel (%d, %d)" % (what, I // 2, J // 2))
            if positive and Wd <= 0:
                raise ValueError("quads: %s: the horizon crosses the rectified crop" % what)
    return m


def quad_matrices(quad, scale: int = 1):
    """one checked quad, the up-scaling factor -> (m_rectify, m_paste, (bx0, by0, bx1, by1)): nine ints each, row-major.
    m_rectify warps the scene into the (bh, bw) crop; m_paste warps the (scale * bh, scale * bw) line into the quad's bounding box
    [scale * bx0, scale * bx1) x [scale * by0, scale * by1) of the up-scaled canvas.  ValueError when the integers do not fit."""
    from .polys import _QUAD, _maps
    maps = _maps(quad, scale, True, True, _QUAD)
    return maps.rect[0], maps.paste[0], maps.bbox


# ---- the warp -------------------------------------------------------------------------------------------------------------------------
def _warp_coords(m, out_h, out_w):
    """-> (gx, gy, Wd > 0) per destination pixel, int64 (wrapping like the kernel's arithmetic for matrices no plan would pass)"""
    import numpy as np
    m = [np.int64(v) for v in m]
    J = 2 * np.arange(out_w, dtype=np.int64)[None, :] + 1
    I = 2 * np.arange(out_h, dtype=np.int64)[:, None] + 1
    with np.errstate(over="ignore"):
        X, Y, Wd = (m[3 * r] * J + m[3 * r + 1] * I + m[3 * r + 2] for r in range(3))
        ok = Wd > 0
        den = np.where(ok, Wd, 1)
        return np.floor_divide(256 * X, den), np.floor_divide(256 * Y, den), ok


def warp_inside_host(m, out_h, out_w, src_h, src_w):
    """-> the (out_h, out_w) bool mask of the destination pixels a paste (mode 1) paints"""
    gx, gy, ok = _warp_coords(m, out_h, out_w)
    return ok & (gx >= 0) & (gx < 256 * src_w) & (gy >= 0) & (gy < 256 * src_h)


def _sample_host(src, gx, gy, feather=0, old=None):
    """The pixel rule of `warp_u8_host` and `poly_paste_host`, on whole arrays.  src: (H, W, 3) uint8; gx, gy: int64 source coordinates
    in 1 / 256 pixels -> the int64 bilinear sample: fx = gx - 128, x0 = fx >> 8, ax = fx & 255 (fy alike), the four taps clamped to the
    source, the sum rounded at 2^15.  feather = F > 0: blended with `old` (int64, what the target holds): a = min(d + 1, F + 1),
    D = F + 1, d = min(xi, W - 1 - xi, yi, H - 1 - yi) for xi = gx >> 8 clamped to the source (a pixel that is painted has it inside
    anyway, except a polygon's inner strips) and yi = gy >> 8, and the pixel becomes (2 (a new + (D - a) old) + D) // (2 D)."""
    import numpy as np
    hs, ws = src.shape[:2]
    fx, fy = gx - 128, gy - 128
    x0, y0, ax, ay = fx >> 8, fy >> 8, (fx & 255)[:, :, None], (fy & 255)[:, :, None]
    xa, xb = np.clip(x0, 0, ws - 1), np.clip(x0 + 1, 0, ws - 1)
    ya, yb = np.clip(y0, 0, hs - 1), np.clip(y0 + 1, 0, hs - 1)
    p = src.astype(np.int64)
    top = (256 - ax) * p[ya, xa] + ax * p[ya, xb]
    bot = (256 - ax) * p[yb, xa] + ax * p[yb, xb]
    v = ((256 - ay) * top + ay * bot + 32768) >> 16
    if feather:
        xi, yi, D = np.clip(gx >> 8, 0, ws - 1), gy >> 8, feather + 1
        a = (np.minimum(np.minimum(np.minimum(xi, ws - 1 - xi), np.minimum(yi, hs - 1 - yi)), feather) + 1)[:, :, None]
        v = (2 * (a * v + (D - a) * old) + D) // (2 * D)
    return v


def warp_u8_host(src, m, out_h, out_w, dst=None, feather=None):
    """src: (H_src, W_src, 3) uint8, m: nine ints.  dst None: mode 0 -> the (out_h, out_w, 3) uint8 warp, every pixel written.  dst an
    (out_h, out_w, 3) uint8 array: mode 1, the painted pixels are blended INTO dst (in place; also returned) with feather F
    (None = 0): a = min(d + 1, F + 1), D = F + 1, d = min(xi, W_src - 1 - xi, yi, H_src - 1 - yi) for xi = gx >> 8, yi = gy >> 8, and the
    pixel becomes (2 (a new + (D - a) old) + D) // (2 D); every other pixel of dst stays."""
    import numpy as np
    src = np.asarray(src)
    if src.ndim != 3 or src.shape[2] != 3 or src.dtype != np.uint8 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("warp_u8_host takes an (H, W, 3) uint8 source")
    if len(m) != 9 or out_h < 1 or out_w < 1:
        raise ValueError("warp_u8_host takes nine matrix entries and a positive destination size")
    hs, ws = src.shape[:2]
    gx, gy, ok = _warp_coords(m, out_h, out_w)
    if dst is None:
        return np.where(ok[:, :, None], _sample_host(src, gx, gy), 0).astype(np.uint8)
    F = 0 if feather is None else int(feather)
    if F < 0 or dst.shape != (out_h, out_w, 3) or dst.dtype != np.uint8:
        raise ValueError("warp_u8_host: dst must be (out_h, out_w, 3) uint8 and the feather >= 0")
    inside = ok & (gx >= 0) & (gx < 256 * ws) & (gy >= 0) & (gy < 256 * hs)
    dst[inside] = _sample_host(src, gx, gy, F, dst.astype(np.int64))[inside].astype(np.uint8)
    return dst


def quad_rectify_host(scene, quad):
    """RGB PIL image (or an (Hs, Ws, 3) uint8 array), one checked quad -> the (bh, bw, 3) uint8 rectified crop"""
    import numpy as np
    bw, bh = quad_size(quad)
    return warp_u8_host(np.asarray(scene), quad_matrices(quad, 1)[0], bh, bw)


def quad_windows_host(scene, quads, lr_size=(16, 64), stride: int = 32, mask: bool = True):
    """RGB PIL image, quads -> (stack, lines): the concatenation of `line_windows_host(rectified crop, ...)` over the quads, an
    (n_windows, 3 + mask, h, w) float stack, and lines[k] = Line(wl, starts, first window index) of quad k."""
    import numpy as np
    from PIL import Image
    a = np.asarray(scene)
    return _region_windows_host(quad_check(scene.size, quads), lambda quad: Image.fromarray(quad_rectify_host(a, quad), "RGB"), lr_size,
                                stride, mask)


def quad_layers(quads):
    """`scene_layers` on the quads' bounding boxes: pastes of one layer have disjoint destination rectangles"""
    return scene_layers([quad_bbox(q) for q in quads])


def quad_compose_host(scene, quads, line_images, scale: int, feather: int = 0, order=None):
    """-> the RGB PIL image of size (scale * Ws, scale * Hs): the canvas is `scene.resize((scale * Ws, scale * Hs), BICUBIC)`; quad k's
    line image (RGB PIL, or an (H, W, 3) uint8 array) is resized with PIL bicubic to (scale * bw, scale * bh) and warped (mode 1, m_paste
    of `quad_matrices`) into the quad's bounding box of the canvas, in quad order (`order`: another order of the indices, e.g. layer
    after layer).  feather = F >= 0 as `warp_u8_host` states it; an axis-aligned quad gets the bytes `scene_compose_host` gives its box."""
    from PIL import Image
    quads = quad_check(scene.size, quads)
    _scale_check("quads", scale)
    canvas, line = _compose_front(("quads", "quads"), scene, len(quads), line_images, scale, feather)
    for k in (range(len(quads)) if order is None else order):
        bw, bh = quad_size(quads[k])
        _, m, (x0, y0, x1, y1) = quad_matrices(quads[k], scale)
        rect = canvas[scale * y0:scale * y1, scale * x0:scale * x1]
        warp_u8_host(line(k, scale * bw, scale * bh), m, rect.shape[0], rect.shape[1], rect, feather)
    return Image.fromarray(canvas, "RGB")


def super_resolve_quads_host(scene, quads, run_windows, lr_size=(16, 64), stride: int = 32, mask: bool = True, rule: str = "floor",
                             c0: int = 0, feather: int = 0, scale=None):
    """The composition on the host: `quad_windows_host` -> per quad `run_windows` (a callable: the (n, 3 + mask, h, w) windows of ONE
    quad -> their (n, C, H, W) SR windows) -> `blend_windows_host` -> `quad_compose_host`.  The scale is H // h; `scale` must be given
    when there is no quad to take it from (and is checked against the model's otherwise)."""
    return _super_resolve_boxes_host(quad_windows_host, quad_compose_host, ("quads", "quads"), scene, quads, run_windows, lr_size, stride,
                                     mask, rule, c0, feather, scale)


# ---- host halves of the launches ------------------------------------------------------------------------------------------------------
def _words(v):
    """a 64-bit two's complement value as (low, high) int32 words"""
    u = int(v) & 0xFFFFFFFFFFFFFFFF
    lo, hi = u & 0xFFFFFFFF, u >> 32
    return [lo - (1 << 32) if lo >= 1 << 31 else lo, hi - (1 << 32) if hi >= 1 << 31 else hi]


def warp_row(src_off, hs, ws, sp, dst_off, oh, ow, dp, feather, mode, m):
    """one QUAD_DESC-int row of tatt_warp_u8: [source byte offset, H_src, W_src, source pitch, target byte offset, OH, OW, target pitch,
    feather, mode (0 rectify, 1 paste), the nine matrix entries as (low, high) int32 words, 0 x 4]"""
    row = [src_off, hs, ws, sp, dst_off, oh, ow, dp, feather, mode]
    for v in m:
        row += _words(v)
    return row + [0] * (QUAD_DESC - len(row))


def quad_plan(scene, quads, lr_size=(16, 64), stride: int = 32, mask: bool = True, limits=None, slimits=None, qlimits=None):
    """Host half of `DeviceCollator.quad_windows`, without a device: -> QuadPlan(arrays, offsets, warp, resize, desc, lines, upload,
    nbytes, out_floats, quads).  One buffer of nbytes bytes: arrays[0], the (Hs, Ws, 3) uint8 scene, at offsets[0] = 0, further uploaded
    sources behind it, `upload` bytes in all; BEHIND the upload, 16-byte aligned, the regions the device fills: the rectified crop of
    every quad (pitch 3 * bw) and, for a crop beyond `limits` (`line_limits()`), its (h, wl) resized version (pitch 3 * wl).
    warp: (n, QUAD_DESC) rows of ONE tatt_warp_u8 launch (mode 0, scene -> crop); resize: (n', RESIZE_DESC) rows of ONE tatt_resize_u8
    launch (crop -> resized crop) for the crops beyond `limits`; desc: (n_windows, SCENE_DESC) rows of tatt_scene_windows naming the crop
    (or its resized version) as a source of its own, origin (0, 0); quads in input order, windows left to right.  A crop that neither the
    window kernel nor the tiled resampler takes (`slimits` = `scene_limits()`: a down-scale beyond its factor) is rectified and resized
    on the host and uploaded (arrays[1:]): `scene_plan`'s fallback, the same bytes by construction."""
    from .polys import _QUAD, _window_plan
    return QuadPlan(*_window_plan(scene, quads, lr_size, stride, mask, limits, slimits, qlimits, _QUAD,
                                  lambda quad: [(quad_matrices(quad, 1)[0], quad_size(quad)[0])]))


def quad_fill(flat, plan):
    """Write one staging slot: flat: a writable 1-D uint8 array -> (o_warp, o_resize, o_desc, pix, used, total), byte offsets.  Layout:
    warp rows at o_warp = 0 | resize rows | window rows | source i at `pix + plan.offsets[i]` (the scene first), all 16-byte aligned;
    `used` = pix + plan.upload bytes are staged and copied, `total` = pix + plan.nbytes is the size of the device buffer.
    `quad_fill(None, plan)` only computes the offsets."""
    import numpy as np
    o_warp = 0
    o_resize = o_warp + _up(plan.warp.nbytes)
    o_desc = o_resize + _up(plan.resize.nbytes)
    pix = o_desc + _up(plan.desc.nbytes)
    if flat is not None:
        for o, t in ((o_warp, plan.warp), (o_resize, plan.resize), (o_desc, plan.desc)):
            flat[o:o + t.nbytes].view(np.int32)[:] = t.reshape(-1)
        for a, o in zip(plan.arrays, plan.offsets):
            flat[pix + o:pix + o + a.size] = a.reshape(-1)
    return o_warp, o_resize, o_desc, pix, pix + plan.upload, pix + plan.nbytes


def quad_paste_plan(size, quads, blend_desc, blend_bytes, scale: int, H: int, feather: int = 0, limits=None, qlimits=None):
    """Host half of `DeviceExporter.scene_quads`, without a device: size = (Ws, Hs) of the scene, blend_desc / blend_bytes:
    `blend_plan`'s rows and size for the quads' lines (their uint8 canvases, H rows each, lie at the front of the output buffer) ->
    QuadPastePlan(resize, warp, layers, order, counts, rects, canvas_off, pitch, nbytes).  Behind the line canvases, 16-byte aligned:
    rects[k], the (scale * bh, scale * bw) rectangle of quad k (pitch 3 * scale * bw), then the canvas at canvas_off (pitch
    3 * scale * Ws).  resize: (1 + n, RESIZE_DESC) rows of tatt_resize_u8: row 0 the background (the scene, packed rows at offset 0 of
    ITS buffer, to the canvas), rows 1 .. n in quad order: line canvas -> rectangle (ONE launch).  warp: (n, QUAD_DESC) rows of
    tatt_warp_u8 (mode 1, rectangle -> the quad's bounding box of the canvas, feathered) in paste order `order` = by (layer, index);
    counts[l] quads in layer l: one launch each."""
    import numpy as np
    from .polys import _QUAD, _paste_front
    quads, mats, resize, rects, canvas_off, pitch, nbytes, layers, order, counts = _paste_front(
        size, quads, blend_desc, blend_bytes, scale, H, feather, limits, qlimits if qlimits is not None else quad_limits(), _QUAD,
        lambda quad: quad_matrices(quad, scale))
    warp = []
    for k in order:
        bw, bh = quad_size(quads[k])
        _, m, (x0, y0, x1, y1) = mats[k]
        warp.append(warp_row(rects[k], scale * bh, scale * bw, 3 * scale * bw, canvas_off + scale * y0 * pitch + 3 * scale * x0,
                             scale * (y1 - y0), scale * (x1 - x0), pitch, feather, 1, m))
    return QuadPastePlan(resize, np.array(warp, np.int32).reshape(-1, QUAD_DESC), layers, order, counts, rects, canvas_off, pitch, nbytes)
