"""Integer specification of the device collate kernel (tatt_amd/csrc/collate.hip): a plain numpy restatement of what Pillow does for
`Image.resize(size, Image.BICUBIC)` on an RGB uint8 image (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal then the
vertical 8-bit pass), of `convert("L")`, and of the mean threshold of `tatt_amd.io.resize_normalize(..., mask=True)`.  The kernel follows
this file step by step; tests/test_collate_device.py holds this file to the installed Pillow, so a Pillow that resamples differently
shows up here before any kernel is blamed."""
import math

import numpy as np

PRECISION_BITS = 22


def bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size: int, out_size: int):
    """-> (kk (out_size, ksize) int64 fixed-point weights, bounds (out_size, 2): first source sample and count).  Python floats are IEEE
    doubles evaluated one operation at a time (no fused multiply-add), like the C code Pillow ships."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int64)
    bounds = np.zeros((out_size, 2), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:                                   # summed in index order
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))   # int(): towards zero
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def resample_axis1(a: np.ndarray, out_size: int) -> np.ndarray:
    """one 8-bit pass along axis 1 of (H, W, C) uint8; a pass to the size the axis already has is skipped, as in Pillow"""
    H, W, C = a.shape
    if out_size == W:
        return a
    kk, bounds = coeffs(W, out_size)
    out = np.empty((H, out_size, C), np.uint8)
    ai = a.astype(np.int64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + (ai[:, xmin:xmin + n, :] * kk[xx, :n][None, :, None]).sum(1)
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)           # arithmetic shift
    return out


def resize_bicubic(a: np.ndarray, size) -> np.ndarray:
    """(H, W, 3) uint8, size = (width, height) -> (height, width, 3) uint8: horizontal pass, then vertical pass"""
    w, h = size
    a = resample_axis1(a, w)
    return resample_axis1(a.transpose(1, 0, 2), h).transpose(1, 0, 2)


def luma(rgb: np.ndarray) -> np.ndarray:
    r = rgb.astype(np.int64)
    return (r[..., 0] * 19595 + r[..., 1] * 38470 + r[..., 2] * 7471 + 0x8000) >> 16


def mask_plane(rgb: np.ndarray) -> np.ndarray:
    """255 where the gray value does not exceed the mean gray value, in integers: L * N <= sum(L)"""
    L = luma(rgb)
    return np.where(L * L.size <= L.sum(), 255, 0).astype(np.uint8)


def to_float(u8: np.ndarray) -> np.ndarray:
    return u8.astype(np.float32) / np.float32(255)


def resize_normalize_ref(a: np.ndarray, size, mask: bool = True) -> np.ndarray:
    """what `io.resize_normalize(Image.fromarray(a), size, mask)` returns, as a (3 + mask, height, width) float32 array"""
    r = resize_bicubic(a, size)
    planes = [r[..., c] for c in range(3)] + ([mask_plane(r)] if mask else [])
    return to_float(np.stack(planes, 0))


# ---- seeded image content shared by the CPU and the GPU tests --------------------------------------------------------------------
def make_image(rng, h: int, w: int, kind: int) -> np.ndarray:
    """kind 0: smooth (a 3 x 5 colour grid stretched bilinearly), 1: noise, 2: two-level, text-like"""
    from PIL import Image
    if kind == 0:
        base = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
        return np.asarray(Image.fromarray(base, "RGB").resize((w, h), Image.BILINEAR)).copy()
    if kind == 1:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 1), dtype=np.uint8) * 200 + 20).repeat(3, 2).astype(np.uint8)


def make_batch(seed: int, B: int = 48):
    """B samples (img_HR, img_lr, img_HRy, img_lry, label) of PIL RGB images: LR 8-39 x 24-159 pixels, HR twice that, content kinds in
    turn; the Y members are further images of the same sizes"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    letters = "abcdefghijklmnopqrstuvwxyz0123456789"
    samples = []
    for b in range(B):
        h, w = int(rng.integers(8, 40)), int(rng.integers(24, 160))
        im = lambda hh, ww, kind: Image.fromarray(make_image(rng, hh, ww, kind % 3), "RGB")
        word = "".join(letters[int(i)] for i in rng.integers(0, len(letters), int(rng.integers(0, 12))))
        samples.append((im(2 * h, 2 * w, b), im(h, w, b + 1), im(2 * h, 2 * w, b + 2), im(h, w, b), word))
    return samples
