"""Text lines of any width through a generator that knows one LR size (csrc/lines.hip; `DeviceCollator.windows`, `DeviceExporter.lines`,
`infer.SuperResolver(long_lines=True)`).

The generators are trained on word crops resized to one LR size (16 x 64).  A text line, a sign or a licence plate squeezed into that size
loses its characters; here the line is resized to the window height at its OWN aspect ratio, cut into overlapping windows of the LR size,
every window is super-resolved like a training crop, and the SR windows are merged with tent weights into one image.

This module is the specification on the host, pure PIL / numpy, and the yardstick of the kernels: every step around the model is integer
arithmetic on uint8, so the device path equals it bit for bit.
* `line_plan`: the line's width `wl` at the window height and the window starts.
* `line_windows_host`: the window stack the model reads (resize, crop, ToTensor, the mask plane of each WINDOW).
* `blend_windows_host`: quantise the SR windows and merge them, a weighted mean in integers rounded half up.
* `super_resolve_lines_host`: the composition, with the model as a callable.
* `line_limits` / `lines_plan` / `blend_plan`: the host halves of the two launches (tatt_line_windows, tatt_line_blend).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

LINE_DESC = 12            # ints per window row of tatt_line_windows (include/tatt_hip.h)
BLEND_DESC = 8            # ints per line row of tatt_line_blend
LINE_MAX_WL = 4096        # widest line at the window height (`line_plan` raises beyond it; tatt_line_limits reports the same)
_ALIGN = 16

Line = namedtuple("Line", "wl starts first")          # one line of a window stack: its width, its window starts, its first window's index


def line_plan(size, lr_size=(16, 64), stride: int = 32):
    """size = (Ws, Hs) of the image, lr_size = (h, w) of the LR window -> (wl, starts): wl = max(w, round-half-up(Ws * h / Hs)), the
    line's width at height h, never below one window; starts: the windows' first columns, `stride` apart, the last one flush right.
    With w / 2 <= stride <= w (anything else raises ValueError) every column lies in at least one and at most three windows."""
    ws, hs = int(size[0]), int(size[1])
    h, w = int(lr_size[0]), int(lr_size[1])
    if ws < 1 or hs < 1 or h < 1 or w < 1:
        raise ValueError("line_plan: sizes must be positive; got image %s, window %s" % ((ws, hs), (h, w)))
    if not (isinstance(stride, int) and w <= 2 * stride and stride <= w):
        raise ValueError("line_plan: stride must be an int in [w / 2, w] = [%g, %d]; got %r" % (w / 2, w, stride))
    wl = max(w, (2 * ws * h + hs) // (2 * hs))
    if wl > LINE_MAX_WL:
        raise ValueError("line_plan: the line is %d columns wide at height %d; at most LINE_MAX_WL = %d" % (wl, h, LINE_MAX_WL))
    if wl == w:
        return wl, [0]
    n = 1 + -(-(wl - w) // stride)
    return wl, [k * stride for k in range(n - 1)] + [wl - w]


def line_windows_host(img, lr_size=(16, 64), stride: int = 32, mask: bool = True):
    """RGB PIL image -> the (n, 3 + mask, h, w) float stack of its windows: `line = img.resize((wl, h), BICUBIC)`, window k is
    `line.crop((x_k, 0, x_k + w, h))` through ToTensor; with `mask` the fourth plane is 1 where the gray value does not exceed the
    WINDOW's mean gray, as `resize_normalize` thresholds a training crop (not the line's mean)."""
    import numpy as np
    from PIL import Image
    from .io import _to_tensor
    h, w = lr_size
    wl, starts = line_plan(img.size, lr_size, stride)
    line = img.resize((wl, h), Image.BICUBIC)
    out = []
    for x in starts:
        win = line.crop((x, 0, x + w, h))
        t = _to_tensor(win)
        if mask:
            m = win.convert("L")
            thres = np.array(m).mean()
            t = torch.cat((t, _to_tensor(m.point(lambda v: 0 if v > thres else 255))), 0)
        out.append(t)
    return torch.stack(out)


def _blend_geometry(H, W, scale, starts, wl):
    if scale < 1 or W % scale or H % scale:
        raise ValueError("blend: scale %r does not divide the SR window %d x %d" % (scale, H, W))
    w = W // scale
    starts = [int(x) for x in starts]
    if not starts or starts[0] != 0 or starts[-1] != wl - w or any(b <= a or b - a > w for a, b in zip(starts, starts[1:])):
        raise ValueError("blend: window starts %s do not cover a line of %d columns with windows of %d" % (starts, wl, w))
    return w, starts


def blend_windows_host(sr, starts, wl: int, scale: int, rule: str = "floor", c0: int = 0):
    """sr: the float (n, C, H, W) SR windows of one line (any device), W = scale * w -> the (H, scale * wl, 3) uint8 canvas of channels
    c0 .. c0 + 2.  Every window is quantised with `quantize_u8(., rule)`; canvas column X takes every window k with
    scale * x_k <= X < scale * x_k + W at its local column j = X - scale * x_k with the integer tent weight wt = min(j + 1, W - j), and
    the pixel is (2 N + D) // (2 D), N = sum wt * v, D = sum wt: the weighted mean rounded half up.  `starts` is the plan's list."""
    import numpy as np
    from .io import quantize_u8
    n, C, H, W = sr.shape
    w, starts = _blend_geometry(H, W, scale, starts, wl)
    if len(starts) != n:
        raise ValueError("blend: %d windows for %d starts" % (n, len(starts)))
    if c0 < 0 or c0 + 3 > C:
        raise ValueError("blend: channels %d .. %d of %d" % (c0, c0 + 2, C))
    q = quantize_u8(np.transpose(sr[:, c0:c0 + 3].detach().cpu().numpy(), (0, 2, 3, 1)), rule).astype(np.int64)      # (n, H, W, 3)
    j = np.arange(W)
    wt = np.minimum(j + 1, W - j)
    num, den = np.zeros((H, scale * wl, 3), np.int64), np.zeros(scale * wl, np.int64)
    for k, x in enumerate(starts):
        num[:, scale * x:scale * x + W] += q[k] * wt[None, :, None]
        den[scale * x:scale * x + W] += wt
    den = den[None, :, None]
    return ((2 * num + den) // (2 * den)).astype(np.uint8)


def sr_scale(H, W, h, w):
    """the (H, W) SR window of an (h, w) LR window -> the model's integer scale; ValueError where the two sides do not agree on one"""
    if H % h or W % w or H // h != W // w:
        raise ValueError("the SR windows %d x %d are no integer multiple of the LR window %d x %d" % (H, W, h, w))
    return H // h


def super_resolve_lines_host(images, run_windows, lr_size=(16, 64), stride: int = 32, mask: bool = True, rule: str = "floor", c0: int = 0,
                             out_sizes=None):
    """The composition on the host: per RGB PIL image `line_windows_host` -> `run_windows` (a callable: (n, 3 + mask, h, w) window stack
    -> (n, C, H, W) SR windows) -> `blend_windows_host` -> one RGB PIL image of size (scale * wl, H) per input, scale = H // h; with
    out_sizes[i] = (width, height) the finished line is resized by PIL."""
    from PIL import Image
    h, w = lr_size
    out = []
    for i, img in enumerate(images):
        wl, starts = line_plan(img.size, lr_size, stride)
        sr = run_windows(line_windows_host(img, lr_size, stride, mask))
        im = Image.fromarray(blend_windows_host(sr, starts, wl, sr_scale(*sr.shape[2:], h, w), rule, c0), "RGB")
        if out_sizes is not None and tuple(out_sizes[i]) != im.size:
            im = im.resize(tuple(out_sizes[i]), Image.BICUBIC)
        out.append(im)
    return out


def _super_resolve_boxes_host(windows_host, compose_host, what, scene, boxes, run_windows, lr_size, stride, mask, rule, c0, feather, scale):
    """`super_resolve_scene_host` and `super_resolve_quads_host` around their own `*_windows_host` and `*_compose_host`;
    what = (the prefix of their messages, their word for a box)"""
    from PIL import Image
    stack, lines = windows_host(scene, boxes, lr_size, stride, mask)
    images = []
    for ln in lines:
        sr = run_windows(stack[ln.first:ln.first + len(ln.starts)])
        s = sr_scale(*sr.shape[2:], *lr_size)
        if scale is not None and scale != s:
            raise ValueError("%s: scale %r given, the model's is %d" % (what[0], scale, s))
        scale = s
        images.append(Image.fromarray(blend_windows_host(sr, ln.starts, ln.wl, scale, rule, c0), "RGB"))
    if scale is None:
        raise ValueError("%s: no %s and no scale" % what)
    return compose_host(scene, boxes, images, scale, feather)


def _region_windows_host(regions, crop, lr_size, stride, mask):
    """`scene_windows_host`, `quad_windows_host` and `poly_windows_host` around crop(region), the RGB PIL crop of one checked region:
    -> (stack, lines), the concatenation of `line_windows_host(crop, ...)` over the regions and lines[k] = Line(wl, starts, first window
    index) of region k"""
    import torch
    h, w = lr_size
    parts, lines, first = [], [], 0
    for region in regions:
        image = crop(region)
        wl, starts = line_plan(image.size, lr_size, stride)
        parts.append(line_windows_host(image, lr_size, stride, mask))
        lines.append(Line(wl, starts, first))
        first += len(starts)
    stack = torch.cat(parts) if parts else torch.zeros(0, 3 + int(bool(mask)), h, w)
    return stack, lines


def _scale_check(who, scale):
    if not (isinstance(scale, int) and not isinstance(scale, bool) and scale >= 1):
        raise ValueError("%s: scale must be a positive int; got %r" % (who, scale))


def _compose_front(what, scene, n, line_images, scale, feather):
    """`scene_compose_host`, `quad_compose_host` and `poly_compose_host` behind their checks of the regions and the scale, in front of
    their own pastes; what as `_super_resolve_boxes_host` takes it, n regions -> (canvas, line): the (scale * Hs, scale * Ws, 3) uint8
    array of the up-scaled scene and line(k, ow, oh), line image k (RGB PIL, or an (H, W, 3) uint8 array) brought to (ow, oh) by PIL
    bicubic, as an array"""
    import numpy as np
    from PIL import Image
    if not (isinstance(feather, int) and not isinstance(feather, bool) and feather >= 0):
        raise ValueError("%s: feather must be an int >= 0; got %r" % (what[0], feather))
    if len(line_images) != n:
        raise ValueError("%s: %d line images for %d %s" % (what[0], len(line_images), n, what[1]))
    if scene.mode != "RGB":
        raise ValueError("%s: an RGB PIL image is taken; got %r" % (what[0], scene.mode))
    ws, hs = scene.size
    canvas = np.array(scene if scale == 1 else scene.resize((scale * ws, scale * hs), Image.BICUBIC))

    def line(k, ow, oh):
        im = line_images[k]
        im = im if isinstance(im, Image.Image) else Image.fromarray(np.ascontiguousarray(im), "RGB")
        return np.asarray(im if im.size == (ow, oh) else im.resize((ow, oh), Image.BICUBIC))
    return canvas, line


# ---- host halves of the launches ------------------------------------------------------------------------------------------------------
def line_limits():
    """tatt_line_limits: {'rows', 'cols', 'wl', 'h', 'w', 'inter_bytes', 'table_bytes', 'windows'} -- the sources the device resampler
    takes (a larger one is resized to (wl, h) by PIL on the host and only cut and converted on the device), the widest line, the largest
    window and the most windows of one line.  A host-only entry: needs no GPU."""
    import ctypes
    from ._lib import LIB
    out = (ctypes.c_int * 8)()
    if LIB.tatt_line_limits(out) != 0:
        raise RuntimeError("tatt_line_limits failed")
    return dict(zip(("rows", "cols", "wl", "h", "w", "inter_bytes", "table_bytes", "windows"), (int(v) for v in out)))


def _resample_taps(n_in, n_out):
    """Pillow's ksize of a pass from n_in to n_out samples (csrc/pil_resample.h col_ksize)"""
    return int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def _line_takes(hs, ws, h, wl, w, lim):
    if hs > lim["rows"] or ws > lim["cols"]:
        return False
    return ws == wl or (hs * w * 3 <= lim["inter_bytes"] and w * _resample_taps(ws, wl) * 4 <= lim["table_bytes"])


def lines_plan(images, lr_size=(16, 64), stride: int = 32, mask: bool = True, limits=None):
    """Host half of `DeviceCollator.windows`, without a device: images: RGB PIL images -> (arrays, desc, lines, nbytes, out_floats):
    arrays[i] the (H, W, 3) uint8 pixels of LINE i (an image beyond `limits` is replaced by its PIL-resized (wl, h) version, which the
    device then only cuts and converts: exact by construction, the fallback of `collate_plan`); desc (n_windows, LINE_DESC) int32 rows
    [source byte offset (16-byte aligned; all windows of a line share it), H_src, W_src, h, wl, x0, w, mask, float offset of the window's
    planes, 0, 0, 0], lines in input order, windows left to right; lines[i] = Line(wl, starts, first window index)."""
    import numpy as np
    from PIL import Image
    lim = limits if limits is not None else line_limits()
    h, w = int(lr_size[0]), int(lr_size[1])
    if not (1 <= h <= lim["h"] and 1 <= w <= lim["w"]):
        raise ValueError("tatt_line_windows takes windows up to %d x %d (got %d x %d)" % (lim["h"], lim["w"], h, w))
    arrays, rows, lines, off, out_off, planes = [], [], [], 0, 0, 3 + int(bool(mask))
    for i, img in enumerate(images):
        if getattr(img, "mode", None) != "RGB":
            raise ValueError("DeviceCollator takes RGB PIL images (Image.open(..).convert('RGB')); item %d is %r" % (
                i, getattr(img, "mode", type(img).__name__)))
        wl, starts = line_plan(img.size, (h, w), stride)
        if wl > lim["wl"] or len(starts) > lim["windows"]:
            raise ValueError("tatt_line_windows takes lines up to %d columns and %d windows (item %d: %d, %d)" % (
                lim["wl"], lim["windows"], i, wl, len(starts)))
        ws, hs = img.size
        if not _line_takes(hs, ws, h, wl, w, lim):
            img = img.resize((wl, h), Image.BICUBIC)
            ws, hs = wl, h
        a = np.asarray(img)
        arrays.append(a)
        lines.append(Line(wl, starts, len(rows)))
        for x in starts:
            rows.append((off, hs, ws, h, wl, x, w, int(bool(mask)), out_off, 0, 0, 0))
            out_off += planes * h * w
        off += -(-a.size // _ALIGN) * _ALIGN
        if off >= 2 ** 31 or out_off >= 2 ** 31:
            raise ValueError("DeviceCollator: the lines do not fit 32-bit offsets")
    return arrays, np.array(rows, np.int32).reshape(-1, LINE_DESC), lines, off, out_off


def lines_fill(flat, arrays, desc):
    """Write one staging slot: flat: a writable 1-D uint8 array -> (pix, used).  Layout: descriptor table at 0 | the pixels of line i at
    `pix +` its rows' offset, both 16-byte aligned; `lines_fill(None, ...)` only computes the offsets."""
    import numpy as np
    pix = -(-desc.nbytes // _ALIGN) * _ALIGN
    offs = sorted(set(int(o) for o in desc[:, 0]))
    used = pix + (offs[-1] + -(-arrays[-1].size // _ALIGN) * _ALIGN if arrays else 0)
    if flat is not None:
        flat[:desc.nbytes].view(np.int32)[:] = desc.reshape(-1)
        for a, o in zip(arrays, offs):
            flat[pix + o:pix + o + a.size] = a.reshape(-1)
    return pix, used


def blend_plan(lines, n_windows, H, W, scale, rule: str = "floor", c0: int = 0, limits=None):
    """Host half of `DeviceExporter.lines`, without a device: lines: the Line records of a (n_windows, C, H, W) SR stack ->
    (desc, starts, nbytes): desc (n_lines, BLEND_DESC) int32 rows [first window, windows, wl, scale, rule, c0, byte offset of the canvas
    (16-byte aligned, canvases one after the other), row pitch 3 * scale * wl], starts (n_windows,) int32 the window starts in stack
    order, nbytes the size of the output."""
    import numpy as np
    from .io import _rule_code
    lim = limits if limits is not None else line_limits()
    code = _rule_code(rule)
    desc, starts, off, end, nxt = np.zeros((len(lines), BLEND_DESC), np.int32), [], 0, 0, 0
    for i, ln in enumerate(lines):
        _blend_geometry(H, W, scale, ln.starts, ln.wl)
        if ln.first != nxt or ln.wl > lim["wl"] or len(ln.starts) > lim["windows"]:
            raise ValueError("blend_plan: line %d: windows %d .. out of order, or beyond line_limits()" % (i, ln.first))
        nxt += len(ln.starts)
        pitch = 3 * scale * ln.wl
        desc[i] = (ln.first, len(ln.starts), ln.wl, scale, code, c0, off, pitch)
        starts.extend(ln.starts)
        end = off + H * pitch
        off = -(-end // _ALIGN) * _ALIGN
        if end >= 2 ** 31:
            raise ValueError("DeviceExporter: the lines do not fit 32-bit offsets")
    if nxt != n_windows:
        raise ValueError("blend_plan: the lines hold %d windows, the SR stack %d" % (nxt, n_windows))
    return desc, np.array(starts, np.int32), end
