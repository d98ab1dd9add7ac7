"""Scene images: super-resolve the text boxes of a photograph and paste them back (csrc/scene.hip; `DeviceCollator.scene_windows`,
`DeviceExporter.scene`, `infer.SuperResolver.scene`).

A user of a scene-text super-resolver has a photograph and a list of axis-aligned boxes from a detector, and wants the photograph back,
up-scaled, with the text in it restored.  Every box is a text line (`tatt_amd/lines.py`): its crop is resized to the window height at
its own aspect ratio, cut into LR windows, every window is super-resolved, the SR windows are merged with tent weights.  The finished
line is resized into the box's rectangle of the up-scaled scene and laid over it, box after box.

This module is the specification on the host, pure PIL / numpy, and the yardstick of the kernels: everything around the model is
integer arithmetic on uint8, so the device path equals it byte for byte.
* `scene_check`: what a list of boxes must satisfy.
* `scene_windows_host`: the window stack of all boxes, `line_windows_host` of every crop.
* `scene_layers`: which pastes may share a launch.
* `scene_compose_host`: the up-scaled scene with the SR lines pasted in, optionally feathered.
* `super_resolve_scene_host`: the composition, with the model as a callable.
* `scene_limits` / `scene_plan` / `scene_fill` / `paste_plan`: the host halves of the launches (tatt_scene_windows, tatt_resize_u8).
"""
from __future__ import annotations

import numbers
from collections import namedtuple

from .lines import Line, _compose_front, _line_takes, _region_windows_host, _super_resolve_boxes_host, line_limits, line_plan

SCENE_MIN_SIDE = 4        # shortest side of a box: with it no paste shrinks by more than 16 : 1 (one window is 4 : 1, a line 16 rows high)
SCENE_DESC = 16           # ints per window row of tatt_scene_windows (include/tatt_hip.h)
RESIZE_DESC = 16          # ints per item row of tatt_resize_u8
_ALIGN = 16

ScenePlan = namedtuple("ScenePlan", "arrays offsets desc lines nbytes out_floats")
PastePlan = namedtuple("PastePlan", "rows layers order counts canvas_off pitch nbytes")


def _up(n):
    return -(-int(n) // _ALIGN) * _ALIGN


def scene_limits():
    """tatt_scene_limits: {'side', 'boxes', 'tile_h', 'tile_w', 'down', 'feather', 'inter_rows', 'items'} -- the largest side of a source
    or target of the tiled resampler, the most boxes of a scene, the resampler's tile, the largest down-scale factor per axis, the largest
    feather, the rows of intermediate a tile keeps, the most items of one launch.  A host-only entry: needs no GPU."""
    import ctypes
    from ._lib import LIB
    out = (ctypes.c_int * 8)()
    if LIB.tatt_scene_limits(out) != 0:
        raise RuntimeError("tatt_scene_limits failed")
    return dict(zip(("side", "boxes", "tile_h", "tile_w", "down", "feather", "inter_rows", "items"), (int(v) for v in out)))


def scene_check(size, boxes, limits=None):
    """size = (Ws, Hs), boxes: integer (x0, y0, x1, y1) with 0 <= x0 < x1 <= Ws, 0 <= y0 < y1 <= Hs and both sides at least
    SCENE_MIN_SIDE, at most scene_limits()['boxes'] of them -> the boxes as a list of int tuples; anything else raises ValueError naming
    the box."""
    lim = limits if limits is not None else scene_limits()
    ws, hs = int(size[0]), int(size[1])
    if ws < 1 or hs < 1 or ws > lim["side"] or hs > lim["side"]:
        raise ValueError("scene: the image is %d x %d; sides from 1 to %d are taken" % (ws, hs, lim["side"]))
    boxes = list(boxes)
    if len(boxes) > lim["boxes"]:
        raise ValueError("scene: %d boxes; at most %d" % (len(boxes), lim["boxes"]))
    out = []
    for k, box in enumerate(boxes):
        try:
            ok = len(box) == 4 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in box)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError("scene: box %d must be four ints (x0, y0, x1, y1); got %r" % (k, box))
        x0, y0, x1, y1 = (int(v) for v in box)
        if not (0 <= x0 < x1 <= ws and 0 <= y0 < y1 <= hs):
            raise ValueError("scene: box %d = %s does not lie in the %d x %d image (0 <= x0 < x1 <= Ws, 0 <= y0 < y1 <= Hs)" % (
                k, (x0, y0, x1, y1), ws, hs))
        if x1 - x0 < SCENE_MIN_SIDE or y1 - y0 < SCENE_MIN_SIDE:
            raise ValueError("scene: box %d = %s is %d x %d; both sides must be at least SCENE_MIN_SIDE = %d" % (
                k, (x0, y0, x1, y1), x1 - x0, y1 - y0, SCENE_MIN_SIDE))
        out.append((x0, y0, x1, y1))
    return out


def scene_windows_host(scene, boxes, lr_size=(16, 64), stride: int = 32, mask: bool = True):
    """RGB PIL image, boxes -> (stack, lines): the concatenation of `line_windows_host(scene.crop(box), ...)` over the boxes, an
    (n_windows, 3 + mask, h, w) float stack, and lines[k] = Line(wl, starts, first window index) of box k.  Every box is a line: a box no
    wider than the LR window's aspect ratio (4 : 1) is one window."""
    return _region_windows_host(scene_check(scene.size, boxes), scene.crop, lr_size, stride, mask)


def scene_layers(boxes):
    """layer[k] = 1 + max(layer[j] for j < k if box j intersects box k), 0 without such a j.  Boxes of one layer are pairwise disjoint
    (of two intersecting boxes the later one lies at least one layer higher), and a box is pasted after every earlier box it touches:
    pasting layer after layer equals pasting box after box."""
    layers = []
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        below = [layers[j] for j, (a0, b0, a1, b1) in enumerate(boxes[:k]) if x0 < a1 and a0 < x1 and y0 < b1 and b0 < y1]
        layers.append(1 + max(below) if below else 0)
    return layers


def _paste_order(boxes):
    """-> (layers, order, counts): `scene_layers` of the boxes, the paste order by (layer, index), the boxes of every layer"""
    layers = scene_layers(boxes)
    order = sorted(range(len(boxes)), key=lambda k: (layers[k], k))
    return layers, order, [layers.count(l) for l in range(max(layers) + 1)] if layers else []


def _feather_weight(oh, ow, feather):
    """a (oh, ow): min(d + 1, F + 1), d the distance to the nearest side of the rectangle"""
    import numpy as np
    i, j = np.arange(oh)[:, None], np.arange(ow)[None, :]
    d = np.minimum(np.minimum(i, oh - 1 - i), np.minimum(j, ow - 1 - j))
    return np.minimum(d + 1, feather + 1)


def scene_compose_host(scene, boxes, line_images, scale: int, feather: int = 0, order=None):
    """-> the RGB PIL image of size (scale * Ws, scale * Hs): the canvas is `scene.resize((scale * Ws, scale * Hs), BICUBIC)`; box k's
    line image (RGB PIL, or an (H, W, 3) uint8 array) is resized with PIL bicubic to (scale * bw, scale * bh) and laid at
    (scale * x0, scale * y0), in box order (`order`: another order of the box indices, e.g. layer after layer).
    feather = F >= 0: a pixel at distance d = min(i, OH - 1 - i, j, OW - 1 - j) from the nearest side of its pasted rectangle takes
    a = min(d + 1, F + 1), D = F + 1 and becomes (2 * (a * new + (D - a) * old) + D) // (2 * D), the rounding of `blend_windows_host`;
    F = 0 is a plain paste."""
    import numpy as np
    from PIL import Image
    boxes = scene_check(scene.size, boxes)
    if not (isinstance(scale, int) and scale >= 1):
        raise ValueError("scene: scale must be a positive int; got %r" % (scale,))
    canvas, line = _compose_front(("scene", "boxes"), scene, len(boxes), line_images, scale, feather)
    D = feather + 1
    for k in (range(len(boxes)) if order is None else order):
        x0, y0, x1, y1 = boxes[k]
        ow, oh = scale * (x1 - x0), scale * (y1 - y0)
        new = line(k, ow, oh).astype(np.int64)
        rect = canvas[scale * y0:scale * y1, scale * x0:scale * x1]
        if feather:
            a = _feather_weight(oh, ow, feather)[:, :, None]
            new = (2 * (a * new + (D - a) * rect.astype(np.int64)) + D) // (2 * D)
        rect[...] = new.astype(np.uint8)
    return Image.fromarray(canvas, "RGB")


def super_resolve_scene_host(scene, boxes, run_windows, lr_size=(16, 64), stride: int = 32, mask: bool = True, rule: str = "floor",
                             c0: int = 0, feather: int = 0, scale=None):
    """The composition on the host: `scene_windows_host` -> per box `run_windows` (a callable: the (n, 3 + mask, h, w) windows of ONE box
    -> their (n, C, H, W) SR windows) -> `blend_windows_host` -> `scene_compose_host`.  The scale is H // h; `scale` must be given when
    there is no box to take it from (and is checked against the model's otherwise)."""
    return _super_resolve_boxes_host(scene_windows_host, scene_compose_host, ("scene", "boxes"), scene, boxes, run_windows, lr_size, stride,
                                     mask, rule, c0, feather, scale)


# ---- host halves of the launches ------------------------------------------------------------------------------------------------------
def scene_plan(scene, boxes, lr_size=(16, 64), stride: int = 32, mask: bool = True, limits=None):
    """Host half of `DeviceCollator.scene_windows`, without a device: -> ScenePlan(arrays, offsets, desc, lines, nbytes, out_floats).
    arrays[0] the (Hs, Ws, 3) uint8 pixels of the scene at offsets[0] = 0; desc (n_windows, SCENE_DESC) int32 rows [byte offset of the
    source image, box height, box width, h, wl, x0 of the window, w, mask, float offset of the window's planes, row pitch in bytes, box
    x0, box y0, 0, 0, 0, 0], boxes in input order, windows left to right.  A box whose crop is beyond `limits` (`line_limits()`: rows,
    columns, bytes of the resampling passes) is resized to (wl, h) by PIL on the host and appended as a source of its own (arrays[1:],
    offsets 16-byte aligned, pitch 3 * wl, origin (0, 0)), which the device then only cuts and converts: the fallback of `lines_plan`."""
    import numpy as np
    from PIL import Image
    lim = limits if limits is not None else line_limits()
    if getattr(scene, "mode", None) != "RGB":
        raise ValueError("DeviceCollator takes RGB PIL images (Image.open(..).convert('RGB')); the scene is %r" % (
            getattr(scene, "mode", type(scene).__name__),))
    boxes = scene_check(scene.size, boxes)
    h, w = int(lr_size[0]), int(lr_size[1])
    if not (1 <= h <= lim["h"] and 1 <= w <= lim["w"]):
        raise ValueError("tatt_scene_windows takes windows up to %d x %d (got %d x %d)" % (lim["h"], lim["w"], h, w))
    a = np.asarray(scene)
    Hs, Ws = a.shape[:2]
    arrays, offsets, rows, lines = [a], [0], [], []
    off, out_off, planes = _up(a.size), 0, 3 + int(bool(mask))
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        bw, bh = x1 - x0, y1 - y0
        wl, starts = line_plan((bw, bh), (h, w), stride)
        if wl > lim["wl"] or len(starts) > lim["windows"]:
            raise ValueError("tatt_scene_windows takes lines up to %d columns and %d windows (box %d: %d, %d)" % (
                lim["wl"], lim["windows"], k, wl, len(starts)))
        if _line_takes(bh, bw, h, wl, w, lim):
            src = (0, bh, bw, 3 * Ws, x0, y0)
        else:
            small = np.asarray(scene.crop((x0, y0, x1, y1)).resize((wl, h), Image.BICUBIC))
            arrays.append(small)
            offsets.append(off)
            src = (off, h, wl, 3 * wl, 0, 0)
            off += _up(small.size)
        lines.append(Line(wl, starts, len(rows)))
        for x in starts:
            rows.append((src[0], src[1], src[2], h, wl, x, w, int(bool(mask)), out_off, src[3], src[4], src[5], 0, 0, 0, 0))
            out_off += planes * h * w
        if off >= 2 ** 31 or out_off >= 2 ** 31:
            raise ValueError("DeviceCollator: the scene does not fit 32-bit offsets")
    if off >= 2 ** 31:
        raise ValueError("DeviceCollator: the scene does not fit 32-bit offsets")
    return ScenePlan(arrays, offsets, np.array(rows, np.int32).reshape(-1, SCENE_DESC), lines, off, out_off)


def scene_fill(flat, plan):
    """Write one staging slot: flat: a writable 1-D uint8 array -> (pix, used).  Layout: descriptor table at 0 | source i at
    `pix + plan.offsets[i]` (the scene first), all 16-byte aligned; `scene_fill(None, plan)` only computes the offsets."""
    import numpy as np
    pix = _up(plan.desc.nbytes)
    used = pix + plan.nbytes
    if flat is not None:
        flat[:plan.desc.nbytes].view(np.int32)[:] = plan.desc.reshape(-1)
        for a, o in zip(plan.arrays, plan.offsets):
            flat[pix + o:pix + o + a.size] = a.reshape(-1)
    return pix, used


def paste_plan(size, boxes, blend_desc, blend_bytes, scale: int, H: int, feather: int = 0, limits=None):
    """Host half of `DeviceExporter.scene`, without a device: size = (Ws, Hs) of the scene, blend_desc / blend_bytes: `blend_plan`'s rows
    and size for the boxes' lines (their uint8 canvases, H rows each, lie at the front of the output buffer), scale, feather ->
    PastePlan(rows, layers, order, counts, canvas_off, pitch, nbytes).  rows (1 + n_boxes, RESIZE_DESC) int32 rows of tatt_resize_u8
    [source byte offset, H_src, W_src, source pitch, target byte offset, OH, OW, target pitch, feather, 0 x 7]: row 0 the background
    (the scene, packed rows at offset 0 of ITS buffer, to the canvas at canvas_off, pitch 3 * scale * Ws, no feather), then one row per
    box in paste order `order` = by (layer, index): line canvas -> the box's rectangle.  counts[l] boxes in layer l: one launch each.
    canvas_off is 16-byte aligned behind the line canvases; nbytes the size of the output buffer."""
    import numpy as np
    lim = limits if limits is not None else scene_limits()
    boxes = scene_check(size, boxes, lim)
    ws, hs = int(size[0]), int(size[1])
    if not (isinstance(scale, int) and scale >= 1):
        raise ValueError("scene: scale must be a positive int; got %r" % (scale,))
    if not (isinstance(feather, int) and not isinstance(feather, bool) and 0 <= feather <= lim["feather"]):
        raise ValueError("scene: feather must be an int in [0, %d]; got %r" % (lim["feather"], feather))
    if len(blend_desc) != len(boxes):
        raise ValueError("scene: %d lines for %d boxes" % (len(blend_desc), len(boxes)))
    if scale * max(ws, hs) > lim["side"]:
        raise ValueError("scene: the canvas %d x %d is beyond the largest side %d" % (scale * ws, scale * hs, lim["side"]))
    canvas_off = _up(blend_bytes)
    pitch = 3 * scale * ws
    nbytes = canvas_off + scale * hs * pitch
    if nbytes >= 2 ** 31 or hs * ws * 3 >= 2 ** 31:
        raise ValueError("DeviceExporter: the scene does not fit 32-bit offsets")
    layers, order, counts = _paste_order(boxes)
    rows = np.zeros((1 + len(boxes), RESIZE_DESC), np.int32)
    rows[0, :9] = (0, hs, ws, 3 * ws, canvas_off, scale * hs, scale * ws, pitch, 0)
    for r, k in enumerate(order):
        x0, y0, x1, y1 = boxes[k]
        d = blend_desc[k]
        lw = int(d[3]) * int(d[2])                                   # scale * wl columns of the line canvas
        oh, ow = scale * (y1 - y0), scale * (x1 - x0)
        if H > lim["down"] * oh or lw > lim["down"] * ow:
            raise ValueError("scene: box %d: pasting %d x %d into %d x %d shrinks by more than %d" % (k, H, lw, oh, ow, lim["down"]))
        rows[1 + r, :9] = (int(d[6]), H, lw, int(d[7]), canvas_off + scale * y0 * pitch + 3 * scale * x0, oh, ow, pitch, feather)
    return PastePlan(rows, layers, order, counts, canvas_off, pitch, nbytes)
