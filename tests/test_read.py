"""CPU: the host specification of reading lines at their own width (tatt_amd/read.py), held to plain loops, to Pillow and to
`io.ctc_greedy_decode`.  The kernels are held to this module by tests/test_read_device_gpu.py."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_ref as R


def test_read_width_table():
    from tatt_amd import read
    wls = (64, 65, 71, 97, 128, 160, 209, 400, 652, 653, 4096)
    assert [read.read_width(wl) for wl in wls] == [100, 120, 120, 160, 200, 260, 340, 640, 1020, 1020, 1020]
    assert [read.read_squeezed(wl) for wl in wls] == [False] * 9 + [True, True]
    for wl in range(1, 700):
        rw = read.read_width(wl)
        assert rw % read.READ_QUANTUM == 0 and 20 <= rw <= read.READ_MAX and rw // 4 + 1 <= 256
        assert rw == read.READ_MAX or (100 * wl <= 64 * rw < 100 * wl + 64 * read.READ_QUANTUM)      # the ceiling, in integers
    assert read.read_width(32, w=32) == 100 and read.read_width(100, w=128) == 80
    with pytest.raises(ValueError):
        read.read_width(0)


def test_read_plan_buckets_and_offsets():
    from tatt_amd import read
    sizes = [(32, 194), (32, 128), (32, 142), (32, 1400), (32, 130), (32, 128)]          # rw 160, 100, 120, 1020, 120, 100
    plan = read.read_plan(sizes, 2)
    assert plan.rws == [160, 100, 120, 1020, 120, 100] and plan.squeezed == [False, False, False, True, False, False]
    assert plan.buckets == [(100, [1, 5]), (120, [2, 4]), (160, [0]), (1020, [3])]      # ascending rw, input order inside
    want, off = {}, 0
    for rw, idx in plan.buckets:
        for i in idx:
            want[i] = off
            off += 32 * rw
    assert plan.offsets == [want[i] for i in range(6)] and plan.floats == off == 32 * (200 + 240 + 160 + 1020)
    assert plan.desc.dtype == np.int32 and plan.desc.shape == (6, read.READ_DESC)
    src = 0
    for i, (h, w) in enumerate(sizes):                                                   # packed sources, 16-byte aligned
        assert plan.desc[i].tolist() == [src, h, w, 3 * w, plan.rws[i], plan.offsets[i], 0, 0]
        src += -(-h * 3 * w // 16) * 16
    rows = [(4096, 32, 128, 400), (16, 64, 256, 768)]                                    # where the lines lie; one scale per line
    plan = read.read_plan(rows, (2, 4))
    assert plan.rws == [100, 100] and plan.desc[:, :4].tolist() == [list(r) for r in rows] and plan.offsets == [0, 3200]
    with pytest.raises(ValueError):
        read.read_plan([(32, 129)], 2)                                                   # the scale does not divide the width
    with pytest.raises(ValueError):
        read.read_plan([(32, 128)], (2, 2))
    assert read.read_plan([], 2).buckets == [] and read.read_plan([], 2).floats == 0


def test_line_luma_against_plain_loops():
    """a 32 x 40 line (wl = 20 at scale 2 would be read at 40; here rw = 60: the horizontal pass enlarges, the vertical one is skipped)
    and a 64 x 40 line (the vertical pass shrinks): Pillow's resize restated by tests/pil_resample_ref.py, the luma in Python integers"""
    from tatt_amd import read
    for hs, rw in ((32, 60), (64, 40), (32, 40)):
        a = R.make_image(np.random.default_rng(hs + rw), hs, 40, 1)
        got = read.line_luma_host(a, rw)
        assert got.shape == (32, rw) and got.dtype == np.float32
        px = np.asarray(Image.fromarray(a, "RGB").resize((rw, 32), Image.BICUBIC))
        assert np.array_equal(px, R.resize_bicubic(a, (rw, 32)))
        k = np.float32(1.0 / 255000.0)
        for y in range(32):
            for x in range(rw):
                n = 299 * int(px[y, x, 0]) + 587 * int(px[y, x, 1]) + 114 * int(px[y, x, 2])
                assert 0 <= n <= 255000 and float(np.float32(n)) == n
                assert got[y, x] == np.float32(n) * k
    assert float(read.line_luma_host(np.full((32, 8, 3), 255, np.uint8), 20).max()) <= 1.0
    with pytest.raises(ValueError):
        read.line_luma_host(np.zeros((32, 40), np.uint8), 20)


def _logits(seed, T, B, C=37):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, C, generator=g) * 3
    x[:, :, 0] += 2.0                                                # blanks between characters
    if T > 3:
        x[0, 0, 0] = x[0, 0].max() + 1.0                             # a blank first
        x[1, 0, 5] = x[1, 0, 9] = x[1, 0].max() + 1.0               # an exact tie: the lower class wins
        x[2, 0] = x[1, 0]                                            # and its repeat is merged
        x[3, 0, 0] = x[3, 0, 7] = x[3, 0].max() + 1.0               # a tie with the blank: the blank wins
    x[:, B - 1] = 0.0
    x[:, B - 1, 0] = 4.0                                             # an all-blank image
    return x


def test_ctc_greedy_read_host_against_greedy_decode():
    from tatt_amd import io, read
    d2a = "-" + io.ALPHABET
    for T, B in ((1, 2), (26, 5), (41, 3), (256, 2)):
        x = _logits(T + B, T, B)
        dec = read.ctc_greedy_read_host(x)
        assert ["".join(d2a[c] for c in d.classes) for d in dec] == io.ctc_greedy_decode(x)
        p = torch.softmax(x.double(), -1)
        for b, d in enumerate(dec):
            assert len(d.classes) == len(d.steps) == len(d.char_conf)
            assert all(s1 > s0 for s0, s1 in zip(d.steps, d.steps[1:])) and all(0 <= s < T for s in d.steps)
            for c, s, q in zip(d.classes, d.steps, d.char_conf):
                assert int(x[s, b].argmax()) == c and (s == 0 or int(x[s - 1, b].argmax()) != c)        # the first step of its run
                assert abs(q - float(p[s, b, c])) < 1e-12
            assert abs(d.conf - float(p[:, b].max(-1).values.min())) < 1e-12
            assert not d.char_conf or d.conf <= min(d.char_conf)
            assert 0.0 < d.conf <= 1.0
        assert dec[B - 1].classes == [] and dec[B - 1].steps == [] and abs(dec[B - 1].conf - float(p[0, B - 1, 0])) < 1e-12
        if T > 3:
            assert dec[0].classes[0] == 5 and dec[0].steps[0] == 1                     # the planted tie reads class 5, once
            assert 2 not in dec[0].steps and 3 not in dec[0].steps


def test_read_lines_host_with_a_stub_recogniser():
    from tatt_amd import io, read
    seen = []

    def run_crnn(x):
        assert x.shape[:3] == (1, 1, 32) and x.dtype == torch.float32
        seen.append(x)
        T = x.shape[3] // 4 + 1
        col = x[0, 0].mean(0)[:4 * (T - 1):4]                        # a "recogniser": the class follows the column's brightness
        out = torch.zeros(T, 1, 37)
        out[torch.arange(T - 1), 0, (col * 36).long().clamp(0, 35) + 1] = 5.0
        out[T - 1, 0, 0] = 5.0
        return out
    rng = np.random.default_rng(3)
    lines = [R.make_image(rng, 32, w, k) for k, w in enumerate((128, 194, 1400))]
    got = read.read_lines_host(lines, run_crnn, scale=2)
    assert [tuple(x.shape) for x in seen] == [(1, 1, 32, 100), (1, 1, 32, 160), (1, 1, 32, 1020)]
    assert [(r.rw, r.squeezed) for r in got] == [(100, False), (160, False), (1020, True)]
    for r, x, a in zip(got, seen, lines):
        assert np.array_equal(x[0, 0].numpy(), read.line_luma_host(a, r.rw))
        d = read.ctc_greedy_read_host(run_crnn(x))[0]
        assert r.chars == d.classes and r.steps == d.steps and r.char_conf == d.char_conf and r.conf == d.conf
        assert r.text == io.ctc_greedy_decode(run_crnn(x))[0] == "".join(("-" + io.ALPHABET)[c] for c in r.chars)
        assert isinstance(r, read.Reading) and r._fields == ("text", "conf", "chars", "char_conf", "steps", "rw", "squeezed")


def test_read_limits_and_the_entries_refuse_without_a_gpu():
    """host-only entries: the limits, and the argument checks that run before any launch"""
    from tatt_amd import read
    from tatt_amd._lib import LIB
    lim = read.read_limits()
    assert lim["height"] == 32 and lim["rw"] == read.READ_MAX and lim["down"] == 16 and lim["desc"] == read.READ_DESC
    assert lim["steps"] == 256 and lim["classes"] == 64 and lim["rw"] // 4 + 1 == lim["steps"]
    assert LIB.tatt_line_luma(None, 0, None, None, 0, None, 0, None) == 1
    # a refused row returns before anything is launched or dereferenced on the device: the codes of the host check, without a GPU
    import ctypes
    fake = ctypes.create_string_buffer(64)                           # stands in for the device pointers: never read

    def run(row, nbytes=16 + 32 * 426, nfloats=32 * 120):
        host = (ctypes.c_int * 8)(*row)
        return LIB.tatt_line_luma(fake, nbytes, fake, host, 1, fake, nfloats, None)
    row = lambda **kw: [kw.get(k, v) for k, v in (("src", 16), ("h", 32), ("w", 142), ("pitch", 426), ("rw", 120), ("out", 0), ("r6", 0),
                                                  ("r7", 0))]
    assert run(row(r6=1)) == 1 and run(row(r7=-1)) == 1
    assert run(row(rw=lim["rw"] + 1)) == 2 and run(row(rw=0)) == 2 and run(row(h=0)) == 2 and run(row(w=0)) == 2
    assert run(row(h=lim["down"] * 32 + 1)) == 2 and run(row(w=lim["down"] * 120 + 1, pitch=3 * (lim["down"] * 120 + 1))) == 2
    assert run(row(w=lim["width"] + 1)) == 2
    assert run(row(src=-1)) == 3 and run(row(pitch=425)) == 3 and run(row(), nbytes=16 + 32 * 426 - 1) == 3
    assert run(row(out=-1)) == 3 and run(row(out=1)) == 3 and run(row(), nfloats=32 * 120 - 1) == 3
    assert LIB.tatt_line_luma(fake, 64, fake, fake, lim["lines"] + 1, fake, 64, None) == 2
    assert LIB.tatt_ctc_greedy_read(None, 0, 0, 0, 26, 1, 37, None, None, 1, 26, 80, None) == 1
