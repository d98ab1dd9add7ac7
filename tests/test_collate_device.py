"""Device collation (tatt_amd.io.DeviceCollator, csrc/collate.hip), the parts that need no GPU: the C ABI, the integer specification the
kernel follows (tests/pil_resample_ref.py) against the installed Pillow, and the host packing pass.  All comparisons are exact."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resample_ref as R

TARGETS = ((128, 32), (64, 16), (256, 64))                  # (width, height)
EDGE_SOURCES = ((1, 1), (1, 7), (5, 1), (16, 64), (32, 128), (16, 128), (32, 64), (33, 129), (15, 63), (256, 1024), (512, 2048))   # (rows, columns)


def test_header_declares_and_library_exports_the_collate_entry_points():
    from tatt_amd._lib import LIB, parse_header
    from tatt_amd.build import EXTRA_FLAGS, SOURCES
    protos = parse_header()
    assert "tatt_collate_images" in protos and "tatt_collate_limits" in protos
    args = [n for _, n in protos["tatt_collate_images"]]
    for a in ("packed", "desc", "desc_host", "n_items", "out", "st"):
        assert a in args, a
    assert "collate.hip" in SOURCES and "-ffp-contract=off" in EXTRA_FLAGS["collate.hip"]
    dll = LIB.load()
    assert hasattr(dll, "tatt_collate_images") and hasattr(dll, "tatt_collate_limits")
    from tatt_amd.io import collate_limits
    lim = collate_limits()
    assert lim["rows"] >= 128 and lim["cols"] >= 512 and lim["inter_bytes"] >= 128 * 128 * 3     # at least 128 x 512 sources
    assert lim["oh"] >= 64 and lim["ow"] >= 256                                                  # the large-tile geometry


def _check(a, size):
    from tatt_amd import io
    want = io.resize_normalize(Image.fromarray(a, "RGB"), size, mask=True).numpy()
    got = R.resize_normalize_ref(a, size, mask=True)
    assert got.dtype == want.dtype and np.array_equal(got, want), (a.shape, size)


def test_specification_equals_pillow_on_seeded_images():
    rng = np.random.default_rng(1)
    n = 0
    for it in range(300):
        h, w = int(rng.integers(4, 70)), int(rng.integers(8, 300))
        a = R.make_image(rng, h, w, it % 3)
        for size in TARGETS:
            _check(a, size)
            n += 1
    assert n == 900


@pytest.mark.parametrize("hw", EDGE_SOURCES, ids=lambda hw: "%dx%d" % hw)
def test_specification_equals_pillow_on_edge_sources(hw):
    rng = np.random.default_rng(hw[0] * 4099 + hw[1])
    for kind in range(3):
        a = R.make_image(rng, hw[0], hw[1], kind)
        for size in TARGETS:
            _check(a, size)


@pytest.mark.parametrize("value", (0, 128, 255))
def test_specification_equals_pillow_on_constant_images(value):
    for hw in ((9, 40), (32, 128), (64, 256), (3, 5)):
        for size in TARGETS:
            _check(np.full(hw + (3,), value, np.uint8), size)


def test_specification_covers_every_byte_value():
    """the uint8 -> float conversion on all 256 values (a 16 x 16 source that is already the target size: both passes skipped)"""
    from tatt_amd import io
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    want = io.resize_normalize(Image.fromarray(a, "RGB"), (16, 16), mask=True).numpy()
    assert np.array_equal(R.resize_normalize_ref(a, (16, 16)), want)
    assert np.array_equal(np.unique(want[0]), (torch.arange(256).float() / 255).numpy())


def _limits():
    from tatt_amd.io import collate_limits
    return collate_limits()


def test_host_packing():
    from tatt_amd import io
    lim = _limits()
    rng = np.random.default_rng(7)
    shapes = [(9, 40), (32, 128), (16, 64), (1, 1), (lim["rows"], 64), (lim["rows"] + 1, 64), (8, lim["cols"] + 1), (40, 130)]
    arrs = [R.make_image(rng, h, w, i % 3) for i, (h, w) in enumerate(shapes)]
    imgs = [Image.fromarray(a, "RGB") for a in arrs]
    sizes = [(128, 32)] * 4 + [(64, 16)] * 4
    arrays, desc, nbytes, out_floats = io.collate_plan(imgs, sizes, mask=True, limits=lim)
    assert desc.dtype == np.int32 and desc.shape == (len(imgs), io.COLLATE_DESC)
    end, out_off = 0, 0
    for i, (a, img, (ow, oh)) in enumerate(zip(arrays, imgs, sizes)):
        off, hs, ws, doh, dow, m, o, _ = (int(v) for v in desc[i])
        assert off % 16 == 0 and off >= end
        end = off + a.size
        assert (doh, dow, m, o) == (oh, ow, 1, out_off)
        out_off += 4 * oh * ow
        h, w = shapes[i]
        beyond = h > lim["rows"] or w > lim["cols"] or (w != ow and h * ow * 3 > lim["inter_bytes"])
        assert beyond == (i in (5, 6))
        if beyond:                                         # the exact fallback: PIL's own resize, both passes marked skipped
            assert (hs, ws) == (oh, ow)
            assert np.array_equal(a, np.asarray(img.resize((ow, oh), Image.BICUBIC)))
        else:
            assert (hs, ws) == (h, w) and np.array_equal(a, np.asarray(img))
        assert a.dtype == np.uint8 and a.shape == (hs, ws, 3)
    assert nbytes >= end and nbytes % 16 == 0 and out_floats == out_off
    _, d3, _, f3 = io.collate_plan(imgs[:2], sizes[:2], mask=False, limits=lim)
    assert d3[:, 5].tolist() == [0, 0] and d3[1, 6] == 3 * 32 * 128 and f3 == 2 * 3 * 32 * 128


def test_collator_plan_orders_the_members():
    """DeviceCollator.plan: items HR x B, lr x B (then HRy x B, lry x B), each with its member's target"""
    from tatt_amd import io
    samples = R.make_batch(3, B=4)
    # (the constructor only checks the device type: nothing is allocated before the first call)
    for yuv in (False, True):
        c = io.DeviceCollator(imgH=32, imgW=128, down_sample_scale=2, mask=True, device="cuda", want_yuv=yuv)
        (arrays, desc, nbytes, out_floats), labels, members = c.plan(samples)
        assert len(arrays) == (16 if yuv else 8) and list(labels) == [s[4] for s in samples]
        order = (0, 1, 2, 3) if yuv else (0, 1)
        for j, m in enumerate(order):
            for b in range(4):
                assert np.array_equal(arrays[4 * j + b], np.asarray(samples[b][m]))
                assert tuple(desc[4 * j + b, 3:5]) == ((32, 128) if m % 2 == 0 else (16, 64))
        assert out_floats == (2 if yuv else 1) * 4 * 4 * (32 * 128 + 16 * 64)


def test_cpu_device_and_non_rgb_images_are_refused():
    from tatt_amd import io
    with pytest.raises(RuntimeError, match="AMD GPU"):
        io.DeviceCollator(device="cpu")
    gray = Image.fromarray(np.zeros((8, 24), np.uint8), "L")
    with pytest.raises(ValueError):
        io.collate_plan([gray], [(128, 32)], mask=True, limits=_limits())
    with pytest.raises(ValueError):
        io.collate_plan([np.zeros((8, 24, 3), np.uint8)], [(128, 32)], mask=True, limits=_limits())


def test_intermediate_bytes_limit_binds_at_the_large_tile_target():
    """at the 256 x 64 target the bytes of the horizontally resampled rows (H_src * OW * 3) bind before the row limit does"""
    from tatt_amd import io
    lim = _limits()
    top = lim["inter_bytes"] // (256 * 3)                 # most rows a source that needs the horizontal pass may have at OW = 256
    assert top < lim["rows"]
    rng = np.random.default_rng(13)
    shapes = [(top, 500), (top + 1, 500), (top, lim["cols"]), (top + 1, 256), (lim["rows"], 256), (top + 1, 255)]
    imgs = [Image.fromarray(R.make_image(rng, h, w, i % 3), "RGB") for i, (h, w) in enumerate(shapes)]
    arrays, desc, _, _ = io.collate_plan(imgs, [(256, 64)] * len(imgs), mask=True, limits=lim)
    fallback = [tuple(int(v) for v in d[1:3]) == (64, 256) for d in desc]
    assert fallback == [False, True, False, False, False, True]       # (a source that already is 256 wide has no horizontal pass)
    for a, img, fb in zip(arrays, imgs, fallback):
        assert np.array_equal(a, np.asarray(img.resize((256, 64), Image.BICUBIC) if fb else img))


def test_slot_fill_layout():
    """the bytes of a staging slot: descriptor table | label_vecs | pixels, each block 16-byte aligned, pixels equal to np.asarray(img)"""
    from tatt_amd import io
    samples = R.make_batch(5, B=6)
    col = io.DeviceCollator(imgH=32, imgW=128, down_sample_scale=2, mask=True, device="cuda", want_yuv=True)
    (arrays, desc, nbytes, _), labels, _ = col.plan(samples)
    vecs, _, _ = io.collate_labels(labels)
    head, pix, used = io.collate_fill(None, arrays, desc, vecs.numpy())
    assert head % 16 == 0 and pix % 16 == 0 and head >= desc.nbytes and pix >= head + vecs.numel() * 4 and used == pix + nbytes
    flat = np.full(used + 64, 0xA5, np.uint8)
    assert io.collate_fill(flat, arrays, desc, vecs.numpy()) == (head, pix, used)
    assert np.array_equal(flat[:desc.nbytes].view(np.int32).reshape(desc.shape), desc)
    assert np.array_equal(flat[head:head + vecs.numel() * 4].view(np.float32), vecs.numpy().reshape(-1))
    images = [s[m] for m in range(4) for s in samples]
    for img, row in zip(images, desc):
        o = pix + int(row[0])
        assert o % 16 == 0
        assert np.array_equal(flat[o:o + int(row[1]) * int(row[2]) * 3].reshape(int(row[1]), int(row[2]), 3), np.asarray(img))
    assert (flat[used:] == 0xA5).all()                                  # nothing beyond the used prefix


def test_slot_is_handed_out_only_after_its_event():
    """the ring discipline itself, without a device: `_slot` waits for the event recorded behind a slot's previous copy before it returns
    that slot, walks the slots in turn, and waits for nothing else while the slots are large enough"""
    from tatt_amd import io
    log = []

    class Ev:
        def __init__(self, k):
            self.k = k

        def synchronize(self):
            log.append(self.k)

    col = io.DeviceCollator(device="cuda", ring=3)
    col._host = [torch.empty(4096, dtype=torch.uint8) for _ in range(3)]
    col._events = [Ev(0), None, Ev(2)]
    got = []
    for _ in range(5):
        before = len(log)
        k, host = col._slot(1000)
        got.append(k)
        assert host is col._host[k]
        assert log[before:] == ([k] if col._events[k] is not None else [])   # waited for this slot's event, and only for it
    assert got == [0, 1, 2, 0, 1] and log == [0, 2, 0]


def test_stage_orders_wait_slot_copy_launch_and_done(monkeypatch):
    """the staging step every entry point goes through, without a device (fake streams and events, host tensors for both buffers): the
    stream waits for the previous call's `done` only when the stream moved; then the slot's own event; then fill, the copy of the used
    prefix and the slot's event; then the caller's launches; then `done` is recorded and `_last` names this stream.  A call that needs
    more device bytes than it uploads (`quad_windows`) sizes slot and device buffer by the larger number and copies only the smaller."""
    from tatt_amd import io
    log, cur, made = [], [None], []

    class Stream:
        def __init__(self, name):
            self.name = name

        def wait_event(self, ev):
            log.append(("wait", self.name, ev.k))

    class Ev:
        def __init__(self):
            self.k = "ev%d" % len(made)
            made.append(self)

        def synchronize(self):
            log.append(("sync", self.k))

        def record(self, stream):
            log.append(("record", self.k, stream.name))

    class DevBuf(torch.Tensor):
        def record_stream(self, stream):
            log.append(("record_stream", stream.name))

    class NoDevice:
        def __init__(self, device):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    def empty(n, dtype=None, pin_memory=False, device=None):
        t = torch.zeros(n, dtype=dtype)
        return t if device is None else t.as_subclass(DevBuf)

    monkeypatch.setattr(torch.cuda, "device", NoDevice)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: cur[0])
    monkeypatch.setattr(torch.cuda, "Event", Ev)
    monkeypatch.setattr(torch, "empty", empty)
    col = io.DeviceCollator(device="cuda", ring=2)

    def call(stream, need, used, v):
        """one `_stage` on `stream` whose fill writes v over the whole slot -> (what it logged, the slot index it took)"""
        cur[0], before = stream, len(log)

        def fill(flat):
            assert flat.dtype == np.uint8 and flat.size >= need
            log.append(("fill", int(col._dev_buf[0])))               # (the device buffer still holds the previous call's bytes)
            flat[:] = v

        def launch(base, hbase):
            k = (col._i - 1) % col.ring
            assert base == col._dev_buf.data_ptr() and hbase == col._host[k].data_ptr()
            assert col._dev_buf.numel() >= need and col._host[k].numel() >= need
            assert (col._host[k] == v).all()                         # the slot was filled, all of it
            assert (col._dev_buf[:used] == v).all() and not (col._dev_buf[used:need] == v).any()     # the used prefix, and only it
            log.append(("launch", k))
            return "out%d" % v
        assert col._stage(need, used, fill, launch) == "out%d" % v
        assert col._last[0] is stream
        return log[before:], (col._i - 1) % col.ring

    A, B = Stream("A"), Stream("B")
    # the first call: nothing to wait for; the slots are allocated, slot 0's event and `done` are made
    assert call(A, 100, 100, 1) == ([("fill", 0), ("record", "ev0", "A"), ("launch", 0), ("record", "ev1", "A")], 0)
    done = col._last[1]
    assert done is made[1] and col._events == [made[0], None]
    # the same stream: no wait on `done`; slot 1 has no event yet; `done` is the same event, recorded again
    assert call(A, 100, 100, 2) == ([("fill", 1), ("record", "ev2", "A"), ("launch", 1), ("record", "ev1", "A")], 1)
    # another stream: it waits for `done` first, then the host for slot 0's own event, and the device buffer is handed to the stream
    assert call(B, 100, 100, 3) == ([("wait", "B", "ev1"), ("sync", "ev0"), ("record_stream", "B"), ("fill", 2), ("record", "ev0", "B"),
                                     ("launch", 0), ("record", "ev1", "B")], 0)
    assert col._last == (B, done)
    # more device bytes than uploaded bytes, beyond the slots: every event in flight is waited for, slots and device buffer are allocated
    # for the LARGER number, the smaller is copied (the asserts of `launch`)
    cap = col._host[0].numel()
    assert call(B, 3 * cap, 200, 4) == ([("sync", "ev0"), ("sync", "ev2"), ("sync", "ev1"), ("fill", 0), ("record", "ev3", "B"),
                                         ("launch", 1), ("record", "ev1", "B")], 1)
    assert all(h.numel() >= 3 * cap for h in col._host) and col._dev_buf.numel() >= 3 * cap and col._last == (B, done)
