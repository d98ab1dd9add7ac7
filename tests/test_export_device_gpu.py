"""Device export on the GPU (tatt_amd.io.DeviceExporter, csrc/export.hip; tatt_amd.infer.SuperResolver).  Yardstick: the host path
`io.export_pil_batch` (numpy + Pillow on the CPU), itself held to tests/export_ref.py and the installed Pillow by
tests/test_export_device.py.  Once the floats are quantised everything is integer arithmetic, so every comparison is exact
(np.array_equal): there is no tolerance in this file."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.fixtures import make_inputs, randomize_state_dict
from tests import export_ref as E
from tests import pil_resample_ref as R

pytestmark = pytest.mark.gpu
STD = dict(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype == np.uint8, (i, g.shape, w.shape)
        assert np.array_equal(g, w), "item %d %s: %d of %d bytes differ, max |diff| %d" % (
            i, g.shape, int((g != w).sum()), g.size, int(np.abs(g.astype(int) - w.astype(int)).max()))


def _sr_like(dev, B, H, W, seed, channels_last=True):
    """values like a generator's output: mostly inside [0, 1], some beyond either end; channels-last strides as the generators return"""
    x = (torch.rand(B, 4, H, W, generator=torch.Generator().manual_seed(seed)) * 1.2 - 0.1).to(dev)
    if channels_last:
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert x.stride(1) == 1 and not x.is_contiguous()
    return x


def _mixed_sizes(B, H, W):
    """per-item targets: up-scaling, down-scaling, width only, height only, native, one-pixel sides"""
    base = [(2 * W, 2 * H), (W // 2, H // 2), (W + 37, H), (W, H + 9), (W, H), (W - 5, H), (W, H - 3), (3 * W // 2, H // 3), (1, 1),
            (1, H), (W, 1), (2 * W - 1, 2 * H + 1)]
    return [base[b % len(base)] for b in range(B)]


@pytest.mark.parametrize("rule", E.RULES)
@pytest.mark.parametrize("channels_last", (True, False), ids=("channels-last", "contiguous"))
def test_sr_batch_equals_the_host_path(dev, rule, channels_last):
    from tatt_amd import io
    x = _sr_like(dev, 48, 32, 128, seed=48, channels_last=channels_last)
    ex = io.DeviceExporter(device=dev, rule=rule)
    for sizes in (None, (256, 64), _mixed_sizes(48, 32, 128)):
        pending = ex(x, sizes)
        got = pending.result()
        assert all(isinstance(g, Image.Image) and g.mode == "RGB" for g in got)
        _same(got, io.export_pil_batch(x, sizes, rule=rule))
    _same(ex(x, None, c0=1).arrays(), io.export_pil_batch(x, None, rule=rule, c0=1))


@pytest.mark.parametrize("rule", E.RULES)
def test_large_tile_equals_the_host_path(dev, rule):
    from tatt_amd import io
    x = _sr_like(dev, 16, 64, 256, seed=16)
    ex = io.DeviceExporter(device=dev, rule=rule)
    for sizes in (None, (512, 128), _mixed_sizes(16, 64, 256)):
        if sizes is not None and not isinstance(sizes, tuple):
            sizes = [(min(w, 512), min(h, 128)) for w, h in sizes]
        _same(ex(x, sizes).result(), io.export_pil_batch(x, sizes, rule=rule))


def test_route_boundaries_equal_the_host_path(dev):
    """every limit of tatt_export_limits: at it, one below, one above (above: exported at the native size, PIL resizes on the host)"""
    from tatt_amd import io
    lim = io.export_limits()
    h, w, oh, ow, inter = lim["h"], lim["w"], lim["oh"], lim["ow"], lim["inter_bytes"]
    top = inter // (ow * 3)
    assert top < h
    # (source H, source W, target (width, height), takes the host fallback)
    cases = [(h, 40, (100, 40), False), (h - 1, 40, (100, 40), False), (h + 1, 40, (100, 40), True),
             (8, w, (300, 16), False), (8, w - 1, (300, 16), False), (8, w + 1, (300, 16), True),
             (16, 64, (ow, oh), False), (16, 64, (ow - 1, oh - 1), False), (16, 64, (ow + 1, oh), True), (16, 64, (ow, oh + 1), True),
             (top, 100, (ow, 32), False), (top - 1, 100, (ow, 32), False), (top + 1, 100, (ow, 32), True),
             (top + 1, ow, (ow, 32), False),                                # no horizontal pass: the intermediate does not count
             (h, w, (w // 2, h // 2), False), (top, w, (w - 1, top), False),  # the largest source, both passes / the widest horizontal one
             (h + 1, w + 1, (w + 1, h + 1), False)]                         # beyond every source limit, at the native size: no pass
    ex = io.DeviceExporter(device=dev, rule="floor")
    for i, (H, W, size, fallback) in enumerate(cases):
        _, resize, _ = io.export_plan(2, H, W, [size, (W, H)], "floor", lim)
        assert resize == [size if fallback else None, None], (H, W, size)
        x = _sr_like(dev, 2, H, W, seed=100 + i, channels_last=bool(i % 2))
        _same(ex(x, [size, (W, H)]).result(), io.export_pil_batch(x, [size, (W, H)], rule="floor"))


@pytest.mark.parametrize("rule", E.RULES)
def test_special_values_equal_the_host_path(dev, rule):
    """below 0, above 1, +-inf, NaN (-> 0), -0.0, every k / 255 and one ulp either side, the half-way points of the round rule"""
    from tatt_amd import io
    a = E.special_batch(B=2)
    x = torch.from_numpy(a).to(dev)
    ex = io.DeviceExporter(device=dev, rule=rule)
    for c0 in (0, 1):
        got = ex(x, None, c0=c0).arrays()
        _same(got, io.export_pil_batch(x, None, rule=rule, c0=c0))
        _same(got, [E.export_ref(a[b, c0:c0 + 3], None, rule) for b in range(2)])
    sizes = [(200, 50), (64, 16)]
    _same(ex(x, sizes).result(), io.export_pil_batch(x, sizes, rule=rule))


@pytest.mark.parametrize("rule", E.RULES)
def test_collator_then_exporter_is_the_identity_on_every_byte(dev, rule):
    from tatt_amd import io
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    a[..., 1] = a[..., 1][::-1]
    a[..., 2] = a[..., 2].T
    im = Image.fromarray(a, "RGB")
    col = io.DeviceCollator(imgH=16, imgW=16, down_sample_scale=1, mask=True, device=dev)
    hr = col([(im, im, im, im, "x")])[0]
    stack = col.stack([im, im], (16, 16))
    assert torch.equal(stack[0], hr[0]) and torch.equal(stack[1], hr[0])
    ex = io.DeviceExporter(device=dev, rule=rule)
    got = ex(hr).arrays()
    assert len(got) == 1 and np.array_equal(got[0], a) and np.unique(got[0][..., 0]).size == 256
    _same(ex(stack).arrays(), [a, a])


def test_collator_stack_equals_resize_normalize(dev):
    from tatt_amd import io
    samples = R.make_batch(77, B=12)
    ims = [s[1] for s in samples]
    for mask in (True, False):
        col = io.DeviceCollator(imgH=16, imgW=64, down_sample_scale=1, mask=mask, device=dev)
        got = col.stack(ims, (64, 16))
        want = torch.stack([io.resize_normalize(im, (64, 16), mask) for im in ims]).to(dev)
        assert got.shape == want.shape and torch.equal(got, want)


def _host_panels(lr, sr, hr, gap, rule):
    from tatt_amd import io
    B, _, H, W = hr.shape
    members = (io.export_pil_batch(lr, (W, H), rule), io.export_pil_batch(sr, None, rule), io.export_pil_batch(hr, None, rule))
    out = []
    for b in range(B):
        canvas = np.zeros((3 * H + 4 * gap, W, 3), np.uint8)
        for m in range(3):
            canvas[m * (H + gap):m * (H + gap) + H] = np.asarray(members[m][b])
        out.append(canvas)
    return out


@pytest.mark.parametrize("gap", (0, 5))
def test_panels_equal_the_host_composition(dev, gap):
    from tatt_amd import io
    lr, sr, hr = _sr_like(dev, 7, 16, 64, 1, False), _sr_like(dev, 7, 32, 128, 2, True), _sr_like(dev, 7, 32, 128, 3, False)
    ex = io.DeviceExporter(device=dev, rule="floor")
    ex(_sr_like(dev, 9, 32, 128, 4)).result()                       # (leaves other bytes in the buffers the panels reuse)
    want = _host_panels(lr, sr, hr, gap, "floor")
    _same(ex.panels(lr, sr, hr, gap=gap).arrays(), want)
    if gap == 0:                                                     # make_grid(nrow=1, padding=0): the three members stacked
        L = io.export_pil_batch(lr, (128, 32), "floor")
        assert np.array_equal(want[3][:32], np.asarray(L[3])) and want[3].shape == (96, 128, 3)
    else:
        assert want[0].shape == (32 * 3 + 20, 128, 3) and not want[0][32:37].any() and not want[0][-10:].any()
    # tripple_display: ToPILImage (floor) on the LR member, save_image (round) on the grid
    mixed = io.DeviceExporter(device=dev, rule="round").panels(lr, sr, hr, gap=gap, lr_rule="floor").arrays()
    wr, wf = _host_panels(lr, sr, hr, gap, "round"), _host_panels(lr, sr, hr, gap, "floor")
    for b in range(7):
        assert np.array_equal(mixed[b][:32], wf[b][:32]) and np.array_equal(mixed[b][32:], wr[b][32:])


def test_three_exports_in_flight_on_a_ring_of_two(dev):
    from tatt_amd import io
    xs = [_sr_like(dev, 48, 32, 128, seed=300 + i) for i in range(3)]
    ex = io.DeviceExporter(device=dev, rule="floor", ring=2)
    ex(xs[0]).result()                                               # (slots allocated)
    assert len(ex._slots) == 2
    pend = [ex(x, (256, 64)) for x in xs]                            # nothing read in between
    assert len(ex._slots) == 3 and all(s.held for s in ex._slots)
    for p, x in reversed(list(zip(pend, xs))):
        _same(p.result(), io.export_pil_batch(x, (256, 64), "floor"))
    assert not any(s.held for s in ex._slots)
    again = ex(xs[1])
    assert len(ex._slots) == 3                                       # a free slot is reused
    _same(again.result(), io.export_pil_batch(xs[1], None, "floor"))


def _generator(dev, seed=1234):
    import tatt_amd
    torch.manual_seed(seed)
    m = tatt_amd.TSRN_TL_TRANS(**STD)
    m.load_state_dict(randomize_state_dict(m.state_dict()))
    return m.to(dev).eval()


def _crnn(dev, seed=5):
    import tatt_amd
    torch.manual_seed(seed)
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=seed))
    return c.to(dev).eval()


def test_export_of_a_session_output_survives_the_next_run(dev):
    """the source is the session's static SR tensor; the next replay overwrites it, but only after the export that was enqueued first"""
    from tatt_amd import io
    from tatt_amd.infer import InferenceSession
    m = _generator(dev)
    s = InferenceSession(m, batch_size=8)
    (x1, tp1, _), (x2, tp2, _) = make_inputs(8, seed=31), make_inputs(8, seed=32)
    ex = io.DeviceExporter(device=dev, rule="floor")
    s.run(x1.to(dev), text_prior=tp1.to(dev))                         # (capture)
    sr = s.run(x1.to(dev), text_prior=tp1.to(dev))[0]
    first = sr.clone()
    x2d, tp2d = x2.to(dev), tp2.to(dev)
    pending = ex(sr, (256, 64))
    sr2 = s.run(x2d, text_prior=tp2d)[0]
    assert sr2.data_ptr() == sr.data_ptr()
    got = pending.result()
    torch.cuda.synchronize()
    assert not torch.equal(sr, first)                                 # the buffer really was overwritten
    _same(got, io.export_pil_batch(first, (256, 64), "floor"))
    assert first.stride(1) == 1 or first.is_contiguous()


def test_c_layer_refuses_what_it_does_not_take(dev):
    """non-zero return codes from the desc_host check, before any launch; never a fallback inside the C layer"""
    from tatt_amd import io, ops
    lim = io.export_limits()
    src = torch.rand(2, 4, 16, 64, device=dev)
    out = torch.zeros(2 * 128 * 512 * 3, dtype=torch.uint8, device=dev)

    def run(row, n=1, dev_row=None, t=src, out_bytes=None):
        host = torch.tensor(row, dtype=torch.int32)
        d = torch.tensor(dev_row if dev_row is not None else row, dtype=torch.int32).to(dev)
        B, C, H, W = t.shape
        return ops.LIB.tatt_export_images(ops.P(t), *t.stride(), B, C, H, W, ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(host.data_ptr()),
                                          n, ops.P(out), out.numel() if out_bytes is None else out_bytes, ops.stream())
    ok = [1, 0, 32, 128, 0, 16, 3 * 128 + 5, 0]
    assert run(ok) == 0
    assert run(ok, n=0) == 1
    assert run([1, 0, 32, 128, 2, 16, 3 * 128, 0]) == 1                               # no such rule
    assert run([1, 0, 32, 128, 0, 16, 3 * 128, 7]) == 1                               # the reserved word
    assert run([0, 0, lim["oh"] + 1, 128, 0, 0, 3 * 128, 0]) == 2
    assert run([0, 0, 32, lim["ow"] + 1, 0, 0, 3 * (lim["ow"] + 1), 0]) == 2
    assert run([0, 0, 0, 128, 0, 0, 3 * 128, 0]) == 2
    tall = torch.zeros(1, 3, lim["inter_bytes"] // (lim["ow"] * 3) + 1, 8, device=dev)
    assert run([0, 0, 32, lim["ow"], 0, 0, 3 * lim["ow"], 0], t=tall) == 2           # the intermediate
    assert run([2, 0, 32, 128, 0, 0, 3 * 128, 0]) == 3                                # no such image
    assert run([0, 2, 32, 128, 0, 0, 3 * 128, 0]) == 3                                # channels 2 .. 4 of four
    assert run([0, -1, 32, 128, 0, 0, 3 * 128, 0]) == 3
    assert run([0, 0, 32, 128, 0, 0, 3 * 128 - 1, 0]) == 3                            # rows would overlap
    assert run([0, 0, 32, 128, 0, -16, 3 * 128, 0]) == 3
    assert run([0, 0, 32, 128, 0, 0, 3 * 128, 0], out_bytes=32 * 128 * 3 - 1) == 3
    assert run([0, 0, 32, 128, 0, 0, 3 * 128, 0], out_bytes=32 * 128 * 3) == 0
    # the kernel re-checks the row it reads from device memory and writes nothing for one it refuses (both rows stay inside `out`)
    out.fill_(7)
    assert run(ok, dev_row=[1, 0, 32, 128, 0, 16, 3 * 128 - 1, 0]) == 0
    assert run(ok, dev_row=[1, 0, 32, 128, 2, 16, 3 * 128 + 5, 0]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_exporter_call_makes_no_host_sync(dev):
    from tatt_amd import io
    x = _sr_like(dev, 48, 32, 128, seed=9)
    lr = _sr_like(dev, 48, 16, 64, seed=10)
    ex = io.DeviceExporter(device=dev, rule="round")
    ex(x, (256, 64)).result()                                        # (buffers allocated, the kernel's attribute set)
    ex.panels(lr, x, x, gap=5).result()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p1 = ex(x, (256, 64))
        p2 = ex(x, _mixed_sizes(48, 32, 128))
        p3 = ex.panels(lr, x, x, gap=5)
        p4 = ex(x)                                                   # every slot held: the ring grows, still without a wait
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same(p1.result(), io.export_pil_batch(x, (256, 64), "round"))
    _same(p2.result(), io.export_pil_batch(x, _mixed_sizes(48, 32, 128), "round"))
    _same(p3.arrays(), _host_panels(lr, x, x, 5, "round"))
    _same(p4.result(), io.export_pil_batch(x, None, "round"))


def _crops(n, seed):
    rng = np.random.default_rng(seed)
    return [Image.fromarray(R.make_image(rng, int(rng.integers(8, 40)), int(rng.integers(24, 160)), i % 3), "RGB") for i in range(n)]


def test_super_resolver_equals_the_host_path_on_its_own_sr(dev):
    """100 crops of mixed sizes at batch_size 48: 48 + 48 + 4, the small last batch in a session of its own"""
    from tatt_amd import io
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.infer import SuperResolver
    m, prior, rec = _generator(dev), _crnn(dev, 5), _crnn(dev, 6)
    crops = _crops(100, seed=41)
    up = SuperResolver(m, prior=prior, recognizer=rec, batch_size=48, lr_size=(16, 64), mask=True, rule="floor", keep_sr=True)
    twice = [(min(2 * im.size[0], 512), min(2 * im.size[1], 128)) for im in crops]
    for out_sizes in (None, twice):
        pending = up(crops, out_sizes)
        images, texts = pending.result()
        assert [t.shape[0] for t in pending.sr] == [48, 48, 4] and sorted(up.sessions) == [4, 48]
        assert len(images) == len(texts) == 100
        want_images, want_texts, lo = [], [], 0
        for sr in pending.sr:
            n = sr.shape[0]
            assert tuple(sr.shape[1:]) == (4, 32, 128)
            want_images += io.export_pil_batch(sr, None if out_sizes is None else out_sizes[lo:lo + n], "floor")
            with torch.no_grad():
                want_texts += io.ctc_greedy_decode(rec(parse_crnn_data(sr[:, :3].contiguous())))
            lo += n
        _same(images, want_images)
        assert [im.size for im in images] == ([(128, 32)] * 100 if out_sizes is None else twice)
        assert texts == want_texts
    # without a recogniser only the images come back
    lean = SuperResolver(m, prior=prior, batch_size=48, keep_sr=True)
    pending = lean(crops[:5])
    images = pending.result()
    assert isinstance(images, list) and len(images) == 5
    _same(images, io.export_pil_batch(pending.sr[0], None, "floor"))


def test_evaluate_session_export_callback(dev):
    from tatt_amd import io
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.infer import evaluate_session
    m, crnn = _generator(dev), _crnn(dev)
    batches = []
    for i, B in enumerate((8, 8, 5)):
        x, tp, hr = make_inputs(B, seed=21 + i)
        hr = hr.clamp(0, 1)
        with torch.no_grad():
            labels = io.ctc_greedy_decode(crnn(parse_crnn_data(hr[:, :3].contiguous().to(dev))))
        batches.append((x.to(dev), hr.to(dev), tp.to(dev), labels))
    plain = evaluate_session(m, batches, recognizer=crnn, voc_type="all")
    seen, kept, sess = {}, {}, {}

    def cb(i, pending):
        assert i not in seen
        seen[i] = pending                                             # kept unread until the evaluation is over
        s = next(v for k, v in sess.items() if k[0] == batches[i][0].shape[0])
        kept[i] = s._out[0].clone()                                   # the batch's SR (same stream: before the next replay)
    got = evaluate_session(m, batches, recognizer=crnn, voc_type="all", sessions=sess, export=cb)
    assert got == plain
    assert sorted(seen) == [0, 1, 2]
    for i, (x, hr, tp, labels) in enumerate(batches):
        panels = seen[i].arrays()
        assert len(panels) == x.shape[0] and panels[0].shape == (3 * 32 + 20, 128, 3)
        _same(panels, _host_panels(x, kept[i], hr, 5, "floor"))
