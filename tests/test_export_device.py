"""Device export (tatt_amd.io.DeviceExporter, csrc/export.hip), the parts that need no GPU: the C ABI, the specification the kernel follows
(tests/export_ref.py on top of tests/pil_resample_ref.py) against the installed Pillow, the host path `export_pil_batch` against the
specification, the host plan and the slot ring.  All comparisons are exact."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import export_ref as E
from tests import pil_resample_ref as R

# (width, height): up- and down-scaling of the sources below, width only, height only, one-pixel sides
TARGETS = ((128, 32), (256, 64), (64, 16), (40, 9), (200, 32), (128, 50), (1, 1), (1, 20), (70, 1), (512, 128))


def test_header_declares_and_library_exports_the_export_entry_points():
    from tatt_amd._lib import LIB, parse_header
    from tatt_amd.build import EXTRA_FLAGS, SOURCES
    protos = parse_header()
    assert "tatt_export_images" in protos and "tatt_export_limits" in protos
    args = [n for _, n in protos["tatt_export_images"]]
    assert args == ["src", "st_n", "st_c", "st_h", "st_w", "B", "C", "H", "W", "desc", "desc_host", "n_items", "out", "out_bytes", "st"]
    assert "export.hip" in SOURCES and "-ffp-contract=off" in EXTRA_FLAGS["export.hip"]
    dll = LIB.load()
    assert hasattr(dll, "tatt_export_images") and hasattr(dll, "tatt_export_limits")
    from tatt_amd.io import export_limits
    lim = export_limits()
    assert lim["h"] >= 64 and lim["w"] >= 256                   # sources up to the large tile's HR
    assert lim["oh"] >= 128 and lim["ow"] >= 512                # targets up to 128 x 512
    assert lim["inter_bytes"] >= 98304                          # 64 x 512 x 3: what binds at that target


def test_shared_resampler_header_is_included_not_copied():
    import os
    from tatt_amd.build import CSRC
    # the tables | the quantiser | the tap loop, the stride forms and the two passes | the window family's layout and body | the tile
    # family's span, layout, tile count and body
    shared = ("col_bicubic(double", "void col_coeffs(", "int col_clip8(", "int col_ksize(",
              "int exp_quant(float",
              "PilRgb pil_taps(", "struct PilPacked", "long pil_at(", "void pil_horizontal(", "void pil_vertical(",
              "struct PilWinLayout", "PilWinLayout pil_win_layout(", "void pil_window_body(",
              "int pil_span(", "struct PilTileLayout", "PilTileLayout pil_tile_layout(", "long pil_tiles(", "void pil_tile_body(")
    # the window limits and the geometry check that lines.hip and scene.hip share: line_limits.h, included by those two alone
    limits = ("#define LIN_THREADS", "#define LIN_MAX_ROWS", "#define LIN_MAX_WL", "#define LIN_MAX_TABLE", "#define LIN_LDS", "bool lin_takes(")
    # what a copy of a pass looks like, whatever it is called: the accumulator's rounding term
    copies = ("1 << (COL_PB - 1)",)
    for name in ("collate.hip", "export.hip", "lines.hip", "scene.hip", "read.hip"):
        txt = open(os.path.join(CSRC, name)).read()
        assert '#include "pil_resample.h"' in txt
        assert ('#include "line_limits.h"' in txt) == (name in ("lines.hip", "scene.hip")), name
        for fn in shared + limits + (copies if name != "export.hip" else ()):  # (export.hip keeps its one-byte-per-thread passes over floats)
            assert fn not in txt, (name, fn)
        assert "SCW_MAX" not in txt
    hdr = open(os.path.join(CSRC, "pil_resample.h")).read()
    for fn in shared:
        assert hdr.count(fn) == (2 if fn == "long pil_at(" else 1), fn      # (pil_at: one overload per stride form)
    assert hdr.count(copies[0]) == 1
    lim = open(os.path.join(CSRC, "line_limits.h")).read()
    for fn in limits:
        assert hdr.count(fn) == 0 and lim.count(fn) == 1, fn
    # collate_kernel runs the shared passes from a body of its own (measured: collate.hip's header); the window kernels run the shared body
    col = open(os.path.join(CSRC, "collate.hip")).read()
    assert "pil_horizontal<COL_THREADS>(" in col and col.count("pil_vertical<COL_THREADS>(") == 2 and "pil_window_body<" not in col
    for name in ("lines.hip", "scene.hip"):
        assert open(os.path.join(CSRC, name)).read().count("pil_window_body<LIN_THREADS>(") == 1, name


def _pil(q, size):
    return np.asarray(Image.fromarray(q, "RGB").resize(size, Image.BICUBIC))


def _as_float(q):
    """(H, W, 3) uint8 -> (3, H, W) float32 that quantises back to q under both rules"""
    return np.ascontiguousarray(q.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


def test_specification_equals_pillow_on_seeded_images():
    rng = np.random.default_rng(3)
    n = 0
    for it in range(60):
        h, w = int(rng.integers(2, 65)), int(rng.integers(2, 257))
        q = R.make_image(rng, h, w, it % 3)
        x = _as_float(q)
        for size in TARGETS:
            for rule in E.RULES:
                assert np.array_equal(E.export_ref(x, size, rule), _pil(q, size)), (h, w, size, rule)
                n += 1
    assert n == 60 * len(TARGETS) * 2


@pytest.mark.parametrize("hw", ((1, 1), (1, 9), (7, 1), (16, 64), (32, 128), (64, 256)), ids=lambda hw: "%dx%d" % hw)
def test_specification_equals_pillow_on_edge_sources(hw):
    rng = np.random.default_rng(hw[0] * 131 + hw[1])
    for kind in range(3):
        q = R.make_image(rng, hw[0], hw[1], kind)
        for size in TARGETS:
            assert np.array_equal(E.export_ref(_as_float(q), size, "floor"), _pil(q, size)), (hw, size)


@pytest.mark.parametrize("value", (0, 128, 255))
def test_specification_equals_pillow_on_constant_images(value):
    for hw in ((9, 40), (32, 128), (64, 256), (3, 5)):
        q = np.full(hw + (3,), value, np.uint8)
        for size in TARGETS:
            assert np.array_equal(E.export_ref(_as_float(q), size, "round"), _pil(q, size)), (hw, size)


def test_every_byte_survives_the_round_trip_under_both_rules():
    """float32(k) / 255 * 255 truncates back to k, with and without the + 0.5: DeviceCollator followed by an export is the identity"""
    k = np.arange(256, dtype=np.uint8)
    x = k.astype(np.float32) / np.float32(255)
    for rule in E.RULES:
        assert np.array_equal(E.quantize(x, rule), k), rule


@pytest.mark.parametrize("rule", E.RULES)
def test_host_path_equals_the_specification(rule):
    from tatt_amd import io
    a = E.special_batch(B=3)
    sv = E.special_values()
    assert np.isnan(sv).any() and np.isinf(sv).any() and (sv < 0).any() and (sv > 1).any() and np.signbit(sv[sv == 0]).any()
    t = torch.from_numpy(a)
    for sizes in (None, [(128, 32), (64, 16), (30, 40)], (100, 20)):
        for c0 in (0, 1):
            got = io.export_pil_batch(t, sizes, rule=rule, c0=c0)
            assert len(got) == 3 and all(g.mode == "RGB" for g in got)
            for b, g in enumerate(got):
                size = None if sizes is None else (sizes if isinstance(sizes, tuple) else sizes[b])
                want = E.export_ref(a[b, c0:c0 + 3], size, rule)
                assert np.array_equal(np.asarray(g), want), (sizes, c0, b)
    # channels-last strides (what the generators return) read the same
    cl = t.contiguous(memory_format=torch.channels_last)
    assert all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(io.export_pil_batch(cl, None, rule), io.export_pil_batch(t, None, rule)))
    # the two rules differ exactly where the fraction of x * 255 reaches one half
    x = torch.tensor([[[[0.3 / 255, 0.5 / 255, 0.7 / 255, 254.6 / 255]]] * 3])
    assert np.asarray(io.export_pil_batch(x, None, "floor")[0])[0, :, 0].tolist() == [0, 0, 0, 254]
    assert np.asarray(io.export_pil_batch(x, None, "round")[0])[0, :, 0].tolist() == [0, 1, 1, 255]
    with pytest.raises(ValueError):
        io.export_pil_batch(t, None, rule="nearest")


def _limits():
    from tatt_amd.io import export_limits
    return export_limits()


def test_plan_offsets_and_pitches():
    from tatt_amd import io
    lim = _limits()
    sizes = [(128, 32), (127, 31), (1, 1), (5, 3), (64, 16), (333, 77)]
    desc, resize, nbytes = io.export_plan(len(sizes), 32, 128, sizes, "round", lim)
    assert desc.dtype == np.int32 and desc.shape == (len(sizes), io.EXPORT_DESC) and resize == [None] * len(sizes)
    end = 0
    for b, (ow, oh) in enumerate(sizes):
        ib, c0, doh, dow, rule, off, pitch, zero = (int(v) for v in desc[b])
        assert (ib, c0, doh, dow, rule, zero) == (b, 0, oh, ow, 1, 0)
        assert off % 16 == 0 and off >= end and pitch >= 3 * ow
        end = off + (oh - 1) * pitch + 3 * ow
    assert nbytes == end
    d0, _, _ = io.export_plan(2, 32, 128, None, "floor", lim, c0=1)
    assert d0[:, 1].tolist() == [1, 1] and d0[:, 4].tolist() == [0, 0] and d0[:, 2:4].tolist() == [[32, 128]] * 2
    with pytest.raises(ValueError):
        io.export_plan(2, 32, 128, [(128, 32)], "floor", lim)
    with pytest.raises(ValueError):
        io.export_plan(1, 32, 128, [(128, 32)], "floor", lim, pitch=[3 * 128 - 1], origin=[0])


def test_plan_falls_back_exactly_above_each_limit():
    """a target beyond the limits is planned at the native size and flagged for PIL; at the limit it is not"""
    from tatt_amd import io
    lim = _limits()

    def fb(H, W, size):
        desc, resize, _ = io.export_plan(1, H, W, [size], "floor", lim)
        flagged = resize[0] is not None
        assert tuple(desc[0, 2:4]) == ((H, W) if flagged else (size[1], size[0]))
        assert resize[0] in (None, size)
        return flagged
    h, w, oh, ow, inter = lim["h"], lim["w"], lim["oh"], lim["ow"], lim["inter_bytes"]
    assert not fb(16, 64, (ow, oh)) and fb(16, 64, (ow + 1, oh)) and fb(16, 64, (ow, oh + 1))            # target rows / columns
    assert not fb(h, 64, (128, 32)) and fb(h + 1, 64, (128, 32))                                          # source rows
    assert not fb(16, w, (128, 32)) and fb(16, w + 1, (128, 32))                                          # source columns
    top = inter // (ow * 3)                                                                               # rows at OW = ow: 64
    assert top < h
    assert not fb(top, 100, (ow, 32)) and fb(top + 1, 100, (ow, 32))                                      # intermediate bytes, by the row
    assert not fb(top + 1, ow, (ow, 32))                                                                  # no horizontal pass: no such limit
    # ... and by the byte: a source whose intermediate is exactly the limit, and a limit one byte below it
    rows, cols = 100, 300
    at = dict(lim, inter_bytes=rows * cols * 3)
    below = dict(lim, inter_bytes=rows * cols * 3 - 1)
    assert io.export_plan(1, rows, 90, [(cols, 32)], "floor", at)[1] == [None]
    assert io.export_plan(1, rows, 90, [(cols, 32)], "floor", below)[1] == [(cols, 32)]
    # the native size is always taken, whatever the source
    assert not fb(h + 40, w + 300, (w + 300, h + 40))


@pytest.mark.parametrize("gap", (0, 5))
def test_panel_geometry(gap):
    from tatt_amd import io
    B, H, W = 3, 32, 128
    height, stride, origins = io.panel_layout(B, H, W, gap)
    assert height == 3 * H + 4 * gap and stride % 16 == 0 and stride >= height * 3 * W
    if gap == 5:
        assert height == 3 * H + 20                       # the eval loop's `+ 20`
    canvas = np.zeros(B * stride, np.uint8)
    for m in range(3):
        assert len(origins[m]) == B
        for b in range(B):
            o = origins[m][b] - b * stride
            assert o == m * (H + gap) * 3 * W            # member m starts at row m * (H + gap) of canvas b: rows 0, H + 5, 2 H + 10
            view = canvas[origins[m][b]:origins[m][b] + H * 3 * W]
            assert not view.any()                         # members do not overlap
            view[:] = 1 + m
    for b in range(B):
        c = canvas[b * stride:b * stride + height * 3 * W].reshape(height, W, 3)
        rows = c[:, 0, 0].tolist()
        want = [1] * H + [0] * gap + [2] * H + [0] * gap + [3] * H + [0] * (2 * gap)
        assert rows == want


def test_exporter_refuses_a_cpu_device_and_bad_sources():
    from tatt_amd import io
    with pytest.raises(RuntimeError, match="AMD GPU"):
        io.DeviceExporter(device="cpu")
    with pytest.raises(ValueError):
        io.DeviceExporter(device="cuda", rule="nearest")
    with pytest.raises(ValueError):
        io.DeviceExporter(device="cuda", ring=0)
    ex = io.DeviceExporter(device="cuda")                 # (the constructor only checks the device type: nothing is allocated)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        ex(torch.zeros(2, 4, 16, 64))
    for bad in (torch.zeros(4, 16, 64), torch.zeros(2, 2, 16, 64), torch.zeros(2, 4, 16, 64, dtype=torch.float64),
                torch.zeros(2, 4, 16, 64, dtype=torch.uint8), np.zeros((2, 4, 16, 64), np.float32)):
        with pytest.raises(ValueError, match="4-D fp32"):
            ex(bad)
    with pytest.raises(ValueError, match="4-D fp32"):
        ex(torch.zeros(2, 4, 16, 64), c0=2)               # channels 2 .. 4 of four


class _Ev:
    def __init__(self, k, log):
        self.k, self.log = k, log

    def synchronize(self):
        self.log.append(self.k)


def test_ring_grows_rather_than_hands_out_a_held_slot():
    """the slot discipline itself, without a device (fake events, ordinary memory for the pinned buffers)"""
    from tatt_amd import io
    ex = io.DeviceExporter(device="cuda", ring=2)
    ex._alloc = lambda n: torch.empty(n, dtype=torch.uint8)
    log = []

    def pending(k):
        slot = ex._slot(1000)
        slot.event = _Ev(k, log)
        slot.host[:19] = k                                # descriptor block (16 bytes) | one 1 x 1 item
        return slot, io.PendingExport(slot, slot.event, 16, [(0, 1, 1, 3, None)])
    s0, p0 = pending(10)
    s1, p1 = pending(11)
    assert s0 is not s1 and s0.held and s1.held and len(ex._slots) == 2
    s2, p2 = pending(12)                                  # both held: a third slot, nobody waited
    assert s2 is not s0 and s2 is not s1 and len(ex._slots) == 3 and log == []
    assert p1.arrays()[0].tolist() == [[[11, 11, 11]]] and log == [11]    # reading waits for its own event, and only for it
    assert not s1.held and s0.held and s2.held
    assert p1.arrays()[0].tolist() == [[[11, 11, 11]]] and log == [11]    # (read once, kept)
    s3, p3 = pending(13)                                  # the slot that was read is the one handed out, without a wait
    assert s3 is s1 and len(ex._slots) == 3 and log == [11]
    p0.release()                                          # released unread: free, but its copy may be in flight
    assert not s0.held
    with pytest.raises(RuntimeError):
        p0.arrays()
    s4, p4 = pending(14)
    assert s4 is s0 and log == [11, 10]                   # waited for the released slot's event before the reuse
    assert len(ex._slots) == 3
    s5, p5 = pending(15)                                  # s0, s1, s2 all held again
    assert len(ex._slots) == 4 and s5 not in (s0, s1, s2)
    for p, k in ((p2, 12), (p3, 13), (p4, 14), (p5, 15)):
        assert p.result()[0].getpixel((0, 0)) == (k, k, k)
    assert not any(s.held for s in ex._slots)
    # a slot too small for the next export is replaced while it is free
    big = ex._slot(1 << 20)
    assert big.host.numel() >= 1 << 20 and big.held
