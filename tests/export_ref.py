"""Specification of the device export kernel (tatt_amd/csrc/export.hip) in numpy: the two quantisation rules of the reference's image
export -- the eval loop's `x * 255`, clip, `astype(np.uint8)` ("floor") and torchvision.utils.save_image's `mul(255).add_(0.5)
.clamp_(0, 255).to(uint8)` ("round") -- with NaN defined as 0, followed by Pillow's bicubic resize as tests/pil_resample_ref.py states it.
Every float operation is one IEEE float32 operation (numpy never fuses a multiply with an add)."""
import numpy as np

from tests import pil_resample_ref as R

RULES = ("floor", "round")


def quantize(a: np.ndarray, rule: str) -> np.ndarray:
    assert rule in RULES
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.multiply(a.astype(np.float32), np.float32(255), dtype=np.float32)
        if rule == "round":
            t = np.add(t, np.float32(0.5), dtype=np.float32)
    q = np.zeros(t.shape, np.uint8)                      # NaN, everything <= 0 (-0.0 and -inf among them)
    mid = (t > 0) & (t < 255)
    q[mid] = np.trunc(t[mid]).astype(np.int64).astype(np.uint8)
    q[t >= 255] = 255                                    # +inf among them
    return q


def export_ref(chw: np.ndarray, size=None, rule: str = "floor") -> np.ndarray:
    """(3, H, W) float32, size = (width, height) or None -> (height, width, 3) uint8"""
    q = np.ascontiguousarray(quantize(chw, rule).transpose(1, 2, 0))
    if size is None or tuple(size) == (q.shape[1], q.shape[0]):
        return q
    return R.resize_bicubic(q, size)


def special_values() -> np.ndarray:
    """float32 values the quantisation must get right: below 0 and above 1, +-inf, NaN, -0.0, every k / 255 (the 256-value identity) and
    the floats one ulp either side of each, the round rule's half-way points"""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    half = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    vals = [k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), half, np.nextafter(half, np.float32(-1)),
            np.nextafter(half, np.float32(2)),
            np.array([-1.0, -1e-3, -1e-30, -0.0, 0.0, 1e-30, 1.0 + 1e-6, 1.5, 2.0, 1e30, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, -np.nan],
                     np.float32)]
    return np.concatenate(vals).astype(np.float32)


def special_batch(B: int = 2, H: int = 32, W: int = 128, seed: int = 5) -> np.ndarray:
    """(B, 4, H, W) float32: every special value in every channel (in different places), the rest uniform in [-0.1, 1.1]"""
    rng = np.random.default_rng(seed)
    sv = special_values()
    a = rng.uniform(-0.1, 1.1, (B, 4, H, W)).astype(np.float32)
    assert sv.size <= H * W
    for b in range(B):
        for c in range(4):
            flat = a[b, c].reshape(-1)
            flat[rng.permutation(H * W)[:sv.size]] = sv
    return a
