"""Reading super-resolved lines at their own width on the GPU (csrc/read.hip; read.LineReader, infer.SuperResolver(reader=...)).
Yardstick: the host specification tatt_amd/read.py (PIL + numpy), itself held to plain loops by tests/test_read.py.  The way into the
recogniser is integer arithmetic and one fp32 multiply: exact (torch.equal).  The decoding's classes, steps and lengths are exact; its
probabilities are fp32 against float64 (bound derived at the test).  The recogniser's logits are held to the float64 oracle by a bound
measured from the eager module's own error.  Shapes: the smallest at which each branch is taken."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests import pil_resample_ref as R
from tests.test_lines_device_gpu import LR, _generator, _img, _same

pytestmark = pytest.mark.gpu
# (H, W) of a uint8 line canvas: vertical pass skipped, rw = 100 | rw = 160 | vertical shrink (scale 4), rw = 100 | two lines of one bucket
# (rw = 120) | the cap: rw = 1020, squeezed | (the last one is uploaded with a pitch beyond 3 W)
LINES = ((32, 128), (32, 194), (64, 256), (32, 142), (32, 142), (32, 1400), (32, 150))
SCALES = (2, 2, 4, 2, 2, 2, 2)
PROB_TOL = 1e-5           # fp32 exp is good to a few ulp and the 37-term sum adds at most about 40 * 2^-24 = 2.4e-6 relative on a value <= 1; about 4 x that


def _upload(dev, arrays, extra_pitch=()):
    """the lines in one uint8 device buffer (filled with a guard value), the first at offset 16 -> (buffer, [(offset, H, W, pitch)])"""
    rows, off = [], 16
    for i, a in enumerate(arrays):
        h, w = a.shape[:2]
        pitch = 3 * w + (extra_pitch[i] if i < len(extra_pitch) else 0)
        rows.append((off, h, w, pitch))
        off += -(-h * pitch // 16) * 16
    flat = np.full(off + 16, 0xA5, np.uint8)
    for a, (o, h, w, pitch) in zip(arrays, rows):
        np.lib.stride_tricks.as_strided(flat[o:], (h, w * 3), (pitch, 1))[:] = a.reshape(h, w * 3)
    return torch.from_numpy(flat).to(dev), rows


def _luma(dev, buf, rows, scales):
    from tatt_amd import read
    plan = read.read_plan(rows, scales)
    out = torch.full((plan.floats + 8,), 7.0, device=dev)
    read.line_luma(buf, torch.from_numpy(plan.desc).to(dev), plan.desc, out[:plan.floats])
    torch.cuda.synchronize()
    assert bool((out[plan.floats:] == 7).all())
    return plan, out[:plan.floats].cpu()


# ---- the way into the recogniser ------------------------------------------------------------------------------------------------------
def test_line_luma_equals_the_host_path(dev):
    from tatt_amd import read
    arrays = [R.make_image(np.random.default_rng(30 + i), h, w, i % 3) for i, (h, w) in enumerate(LINES)]
    extra = (0, 0, 0, 0, 0, 0, 20)
    want = []
    for i, (a, s) in enumerate(zip(arrays, SCALES)):                 # each line in a launch of its own
        buf, rows = _upload(dev, [a], extra[i:i + 1])
        plan, got = _luma(dev, buf, rows, s)
        want.append(torch.from_numpy(read.line_luma_host(a, plan.rws[0])))
        assert got.numel() == 32 * plan.rws[0] and torch.equal(got.view(32, -1), want[-1]), (i, int((got.view(32, -1) != want[-1]).sum()))
    buf, rows = _upload(dev, arrays, extra)                          # all lines in one launch, bucket by bucket in one buffer
    plan, got = _luma(dev, buf, rows, SCALES)
    assert plan.rws == [100, 160, 100, 120, 120, 1020, 120] and plan.squeezed == [False] * 5 + [True, False]
    assert plan.buckets == [(100, [0, 2]), (120, [3, 4, 6]), (160, [1]), (1020, [5])]
    for i, w in enumerate(want):
        g = got[plan.offsets[i]:plan.offsets[i] + w.numel()].view(32, -1)
        assert torch.equal(g, w), (i, int((g != w).sum()))
    foff = 0
    for rw, idx in plan.buckets:                                     # a bucket is one contiguous (n, 1, 32, rw) view
        view = got[foff:foff + len(idx) * 32 * rw].view(len(idx), 1, 32, rw)
        assert torch.equal(view[:, 0], torch.stack([want[i] for i in idx]))
        foff += view.numel()


def test_line_luma_entry_refuses_and_a_stale_row_gives_nan(dev):
    """non-zero return codes from the desc_host check, before any launch; the kernel re-checks the row it reads from device memory: a
    row it refuses fills its own target with NaN and touches nothing else"""
    from tatt_amd import ops, read
    lim = read.read_limits()
    src = torch.randint(0, 256, (16 + 64 * 3 * 256,), dtype=torch.uint8, device=dev)
    out = torch.zeros(3 * 32 * 120, device=dev)

    def run(rows, dev_rows=None, nbytes=None, nfloats=None):
        host = torch.tensor(rows, dtype=torch.int32)
        d = torch.tensor(dev_rows if dev_rows is not None else rows, dtype=torch.int32).to(dev)
        return ops.LIB.tatt_line_luma(ops.P(src), src.numel() if nbytes is None else nbytes, ctypes.c_void_p(d.data_ptr()),
                                      ctypes.c_void_p(host.data_ptr()), len(rows), ops.P(out), out.numel() if nfloats is None else nfloats,
                                      ops.stream())
    row = lambda off=0, **kw: [kw.get(k, v) for k, v in (("src", 16), ("h", 32), ("w", 142), ("pitch", 426), ("rw", 120), ("out", off),
                                                         ("r6", 0), ("r7", 0))]
    assert run([row()]) == 0
    assert run([row(r6=1)]) == 1 and run([row(r7=1)]) == 1
    assert run([row(rw=lim["rw"] + 1)]) == 2 and run([row(rw=0)]) == 2 and run([row(h=0)]) == 2 and run([row(w=0)]) == 2
    assert run([row(h=lim["down"] * 32 + 1, pitch=426)]) == 2 and run([row(w=lim["down"] * 8 + 1, pitch=400, rw=8)]) == 2
    assert run([row(w=lim["down"] * 8, pitch=400, rw=8)]) == 0
    assert run([row(src=-16)]) == 3 and run([row(pitch=425)]) == 3 and run([row()], nbytes=16 + 31 * 426 + 425) == 3
    assert run([row()], nbytes=16 + 31 * 426 + 426) == 0
    assert run([row(off=-1)]) == 3 and run([row(off=2 * 3840 + 1)]) == 3 and run([row()], nfloats=3839) == 3
    out.fill_(7)
    K = 32 * 120
    good = [row(0), row(K), row(2 * K)]
    for stale in (row(K, r6=1), row(K, pitch=425), row(K, src=-16), row(K, h=0), row(K, w=lim["down"] * 120 + 1)):
        out.fill_(7)
        assert run(good, dev_rows=[good[0], stale, good[2]]) == 0
        torch.cuda.synchronize()
        got = out.view(3, 32, 120).cpu()
        assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[2]).any())
        assert not bool((got[0] == 7).any()) and not bool((got[2] == 7).any())
    out.fill_(7)                                                     # a target that lies outside `out`, or no target at all: nothing is written
    assert run([row(0)], dev_rows=[row(2 * K + 1)]) == 0 and run([row(0)], dev_rows=[row(0, rw=lim["rw"] + 1)]) == 0
    assert run([row(0)], dev_rows=[row(-1)]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())


@pytest.mark.parametrize("src_hw,rw", (((11, 37), 40), ((200, 90), 80)), ids=("one-tile-up", "halved-tiles-down"))
def test_line_luma_is_the_luma_of_what_resize_u8_writes(dev, src_hw, rw):
    """the two tile entries share one body and differ in the pixel's sink: tatt_line_luma equals read.py's luma arithmetic on the bytes
    tatt_resize_u8 (feather 0) writes for the same source and target (32, rw), and both equal the host path.  11 x 37 -> 32 x 40 is one
    tile of an up-scale; 200 x 90 -> 32 x 80 shrinks 6.25 : 1 in the vertical, where 32 output rows would name 221 > 192 source rows, so
    the tile height halves to 16: tiles whose first source row is not 0, two tile columns, the second ragged and 16 wide"""
    from tatt_amd import io, ops, read
    lim = io.scene_limits()
    hs, ws = src_hw
    a = R.make_image(np.random.default_rng(hs + ws), hs, ws, 1)
    buf, ((off, _, _, pitch),) = _upload(dev, [a], (11,))
    if hs == 200:                                                    # the case is what the docstring says it is
        span = lambda n: int(np.ceil((n - 1) * hs / 32 + 4 * hs / 32)) + 2
        assert lim["tile_h"] == 32 and span(32) == 221 > lim["inter_rows"] >= span(16) and rw - lim["tile_w"] == 16

    def run(name, row, out):
        host = torch.tensor([row], dtype=torch.int32)
        desc = host.to(dev)
        rc = getattr(ops.LIB, name)(ops.P(buf), buf.numel(), ctypes.c_void_p(desc.data_ptr()), ctypes.c_void_p(host.data_ptr()), 1, ops.P(out),
                                    out.numel(), ops.stream())
        assert rc == 0, (name, rc)
        return out.cpu()
    luma = run("tatt_line_luma", [off, hs, ws, pitch, rw, 0, 0, 0], torch.full((32 * rw,), 7.0, device=dev)).view(32, rw)
    rgb = run("tatt_resize_u8", [off, hs, ws, pitch, 0, 32, rw, 3 * rw, 0] + [0] * 7,
              torch.full((32 * rw * 3,), 7, dtype=torch.uint8, device=dev)).view(32, rw, 3).numpy().astype(np.int32)
    n = 299 * rgb[..., 0] + 587 * rgb[..., 1] + 114 * rgb[..., 2]
    assert torch.equal(luma, torch.from_numpy(n.astype(np.float32) * np.float32(1.0 / 255000.0)))
    assert torch.equal(luma, torch.from_numpy(read.line_luma_host(a, rw)))


# ---- the decoding -------------------------------------------------------------------------------------------------------------------
def _logits(seed, T, B, C=37):
    x = torch.randn(T, B, C, generator=torch.Generator().manual_seed(seed)) * 3
    x[:, :, 0] += 2.0
    if T > 3:
        x[0, 0, 0] = x[0, 0].max() + 1.0
        x[1, 0, 5] = x[1, 0, 9] = x[1, 0].max() + 1.0               # an exact tie: the lower class
        x[2, 0] = x[1, 0]
        x[3, 0, 0] = x[3, 0, 7] = x[3, 0].max() + 1.0               # a tie with the blank
    x[:, B - 1] = 0.0
    x[:, B - 1, 0] = 4.0                                             # an all-blank image
    return x


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("T", (1, 26, 41, 256))
def test_ctc_greedy_read_equals_the_host_decoding(dev, T, B):
    from tatt_amd import read
    wide = torch.zeros(T, B + 2, 64, device=dev)                     # a strided view: the logits are no contiguous tensor
    wide[:, 1:B + 1, 3:40] = _logits(100 * T + B, T, B).to(dev)
    x = wide[:, 1:B + 1, 3:40]
    assert x.stride() == ((B + 2) * 64, 64, 1) and x.storage_offset() == 67          # neither packed nor at the start of its buffer
    cap, n_rows = T + 3, B + 3
    order = [(3 * b + 2) % n_rows for b in range(B)]                 # the scatter: image b writes row order[b]
    assert len(set(order)) == B
    rec = torch.full((n_rows, 3 * cap + 2 + 5), -77, dtype=torch.int32, device=dev)
    read.ctc_greedy_read(x, torch.tensor(order, dtype=torch.int32).to(dev), rec, cap)
    host = rec.cpu()
    want = read.ctc_greedy_read_host(x.cpu())                        # the same logits, copied back
    for r in range(n_rows):
        if r not in order:
            assert bool((host[r] == -77).all()), r
    assert bool((host[:, 3 * cap + 2:] == -77).all())
    got = read.parse_records(host[:, :3 * cap + 2].contiguous(), cap)
    for b, w in enumerate(want):
        g, raw = got[order[b]], host[order[b]]
        assert g.classes == w.classes and g.steps == w.steps and raw[3 * cap] == len(w.classes), (b, g, w)
        assert raw[len(w.classes):cap].eq(-1).all() and raw[cap + len(w.classes):2 * cap].eq(-1).all()
        assert raw[2 * cap + len(w.classes):3 * cap].eq(0).all()
        errs = [abs(a - c) for a, c in zip(g.char_conf + [g.conf], w.char_conf + [w.conf])]
        print("T %d B %d image %d: max |p - p64| = %.3g" % (T, B, b, max(errs)))
        assert max(errs) <= PROB_TOL, (b, errs)
    assert got[order[B - 1]].classes == []
    if T > 3 and B > 1:                                              # (at B = 1 the one image is the all-blank one)
        assert want[0].classes[0] == 5 and want[0].steps[0] == 1 and 2 not in want[0].steps and 3 not in want[0].steps
    from tatt_amd import ops
    bad = lambda **kw: ops.LIB.tatt_ctc_greedy_read(ops.P(x), *x.stride(), kw.get("T", T), B, kw.get("C", 37), ops.P(rec), ops.P(rec),
                                                    n_rows, kw.get("cap", cap), kw.get("st", rec.stride(0)), ops.stream())
    assert bad(T=257) == 1 and bad(C=65) == 1 and bad(cap=T - 1) == 1 and bad(st=3 * cap + 1) == 1 and bad(T=0) == 1


# ---- the recogniser -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


def test_line_reader_logits_against_the_float64_oracle(dev, crnn):
    """One line per rw in (100, 120, 340), read at B = 1 by the eager module, against LineReader(keep_logits=True), which reads the same
    lines together with two more lines of the 120 bucket (so that bucket runs at B = 3).  e = max |eager - float64 oracle|; asserted:
    |reader - float64| <= 4 e + 1e-7 (the factor of the project's drift test: the fold and another batch route are two more rounding
    sources than the eager pass has).  Strings: exactly `ctc_greedy_read_host` of the reader's own logits; against the eager decoding a
    differing step is accepted only where the float64 top-2 margin is below 8 e (none expected).
    Measured on an MI355X (split-bf16 arithmetic): see the README, section "Reading lines"."""
    from oracle import crnn_oracle as O
    from tatt_amd import read
    widths = (128, 142, 418, 130, 150)                               # rw 100, 120, 340, 120, 120
    arrays = [R.make_image(np.random.default_rng(40 + i), 32, w, i % 3) for i, w in enumerate(widths)]
    buf, rows = _upload(dev, arrays)
    reader = read.LineReader(crnn, batch_size=48, keep_logits=True)
    pending = reader.read(buf, rows, 2)
    readings = pending.result()
    assert [r.rw for r in readings] == [100, 120, 340, 120, 120] and [idx for idx, _ in pending.logits] == [[0], [1, 3, 4], [2]]
    mine = {}
    for idx, lg in pending.logits:
        assert lg.shape == (readings[idx[0]].rw // 4 + 1, len(idx), 37)
        for j, i in enumerate(idx):
            mine[i] = lg[:, j:j + 1].cpu()
    sd64 = {k: v.detach().cpu().double() for k, v in crnn.state_dict().items()}
    e = worst = 0.0
    cases = []
    for i in (0, 1, 2):
        x = torch.from_numpy(read.line_luma_host(arrays[i], readings[i].rw)).reshape(1, 1, 32, -1)
        with torch.no_grad():
            eager = crnn(x.to(dev)).cpu()
        ref = O.crnn_forward(sd64, x.double())
        e = max(e, float((eager.double() - ref).abs().max()))
        worst = max(worst, float((mine[i].double() - ref).abs().max()))
        cases.append((i, eager, ref))
    top2 = min(float((lambda s: (s[..., 0] - s[..., 1]).min())(ref.sort(-1, descending=True).values)) for _, _, ref in cases)
    print("eager vs float64 e = %.3g, reader vs float64 = %.3g, smallest float64 top-2 margin = %.3g" % (e, worst, top2))
    assert worst <= 4 * e + 1e-7, (worst, e)
    for i, r in enumerate(readings):                                 # exactly the host decoding of the reader's own logits
        d = read.ctc_greedy_read_host(mine[i])[0]
        assert r.chars == d.classes and r.steps == d.steps and r.text == "".join(("-" + "0123456789abcdefghijklmnopqrstuvwxyz")[c] for c in d.classes)
        assert abs(r.conf - d.conf) <= PROB_TOL and all(abs(a - b) <= PROB_TOL for a, b in zip(r.char_conf, d.char_conf))
    differences = 0
    for i, eager, ref in cases:                                      # against the eager decoding
        a, b = mine[i].argmax(-1)[:, 0], eager.argmax(-1)[:, 0]
        s = ref.sort(-1, descending=True).values[:, 0]
        for t in (a != b).nonzero().flatten().tolist():
            differences += 1
            print("line %d step %d: reader %d, eager %d, float64 margin %.3g" % (i, t, int(a[t]), int(b[t]), float(s[t, 0] - s[t, 1])))
            assert float(s[t, 0] - s[t, 1]) < 8 * e
        if bool((a == b).all()):
            assert readings[i].chars == read.ctc_greedy_read_host(eager)[0].classes
    print("differences against the eager decoding: %d" % differences)


def test_line_reader_follows_the_weights(dev, crnn):
    """the weights contract: a change torch sees is picked up by the next read (re-fold and re-pack), which then agrees with a reader
    built afterwards far better than with its own earlier pass"""
    import copy
    from tatt_amd import read
    c = copy.deepcopy(crnn)
    buf, rows = _upload(dev, [R.make_image(np.random.default_rng(50), 32, 128, 1)])
    reader = read.LineReader(c, keep_logits=True)
    first = reader.read(buf, rows, 2).logits[0][1].clone()
    with torch.no_grad():
        c.cnn.batchnorm2.running_mean.add_(0.05)                     # (bumps the version counter)
    second = reader.read(buf, rows, 2).logits[0][1].clone()
    fresh = read.LineReader(c, keep_logits=True).read(buf, rows, 2).logits[0][1]
    moved, apart = float((first - second).abs().max()), float((second - fresh).abs().max())
    print("the change moved the logits by %.3g; the reader and a fresh one are %.3g apart" % (moved, apart))
    assert moved > 0 and apart <= 0.01 * moved


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
SOURCES = ((16, 64), (16, 97), (23, 301))


@pytest.fixture(scope="module")
def gen(dev):
    return _generator(dev)


def _host_readings(up, dev, lines_u8, scale=2):
    """`read_lines_host` with the reader's own folded forward at B = 1 as the recogniser"""
    from tatt_amd import read
    return read.read_lines_host(lines_u8, lambda x: up.reader.forward(x.to(dev)).cpu(), scale=scale, w=LR[1])


def _same_readings(got, want, probs=True):
    """strings, classes and steps exactly; probs: the probabilities within PROB_TOL -- where the device ran the very forward the host ran
    (a bucket of one line).  A bucket of several lines is another batch, i.e. other kernel routes and roundings in the logits, which the
    decoding's bound does not cover: there only the range is checked."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.text == w.text and g.chars == w.chars and g.steps == w.steps and g.rw == w.rw and g.squeezed == w.squeezed, (i, g, w)
        assert len(g.char_conf) == len(w.char_conf) and 0.0 < g.conf <= min(g.char_conf + [1.0])
        if probs:
            assert abs(g.conf - w.conf) <= PROB_TOL, (i, g.conf, w.conf)
            assert all(abs(a - b) <= PROB_TOL for a, b in zip(g.char_conf, w.char_conf)), i


@pytest.fixture(scope="module")
def reading_lines(dev, gen, crnn):
    from tatt_amd.infer import SuperResolver
    up = SuperResolver(gen, batch_size=8, lr_size=LR, mask=True, rule="floor", keep_sr=True, long_lines=True, stride=32, reader=crnn)
    imgs = [_img(50 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    pending = up(imgs)
    return up, imgs, pending, pending.result()


def test_long_lines_with_a_reader(dev, gen, reading_lines):
    from tatt_amd.infer import SuperResolver
    up, imgs, pending, (images, texts) = reading_lines
    plain = SuperResolver(gen, batch_size=8, lr_size=LR, mask=True, rule="floor", long_lines=True, stride=32)
    _same(images, plain(imgs).result())                              # byte for byte the images without a reader
    readings = pending.readings()
    assert texts == [r.text for r in readings] and len(texts) == 3
    assert [(r.rw, r.squeezed) for r in readings] == [(100, False), (160, False), (340, False)]
    _same_readings(readings, _host_readings(up, dev, [np.asarray(im) for im in images]))
    # out_sizes resize the finished line on the host: the lines were read before
    sized = up(imgs, [(100, 20), (388, 32), (300, 40)])
    im2, tx2 = sized.result()
    assert [im.size for im in im2] == [(100, 20), (388, 32), (300, 40)] and tx2 == texts
    assert up([]).result() == ([], [])


def test_scene_and_scene_quads_with_a_reader(dev, gen, crnn):
    from tatt_amd import io
    from tatt_amd.infer import SuperResolver
    from tests.test_quads_device_gpu import QUADS
    from tests.test_scene_device_gpu import BOXES
    up = SuperResolver(gen, batch_size=4, lr_size=LR, mask=True, rule="floor", keep_sr=True, stride=32, reader=crnn)
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, mask=True, rule="floor", stride=32)
    for scene, regions, run, run_plain in ((_img(60, 48, 160, 1), BOXES, up.scene, plain.scene),
                                           (_img(61, 97, 211, 1), QUADS, up.scene_quads, plain.scene_quads)):
        p = run(scene, regions, 2)
        image = p.result()
        _same([image], [run_plain(scene, regions, 2).result()])      # byte for byte the picture without a reader
        sr = p.sr.cpu()
        blended = [io.blend_windows_host(sr[ln.first:ln.first + len(ln.starts)], ln.starts, ln.wl, 2, "floor") for ln in p.lines]
        texts, readings = p.texts(), p.readings()
        assert len(texts) == len(regions) and texts == [r.text for r in readings]
        assert [r.rw for r in readings] == [io.read_width(ln.wl) for ln in p.lines]
        # one per box, in input order: the reading of the host-blended lines
        _same_readings(readings, _host_readings(up, dev, blended), probs=False)
        none = run(scene, [])
        assert none.texts() == [] and none.readings() == []
        _same([none.result()], [run_plain(scene, []).result()])
    with pytest.raises(RuntimeError, match="reader"):
        plain.scene(_img(60, 48, 160, 1), BOXES[:1]).texts()


def test_second_reading_call_makes_no_host_wait_before_result(dev, reading_lines):
    up, imgs, pending, (images, texts) = reading_lines
    again = [_img(70 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = up(again)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    im2, tx2 = p.result()
    _same_readings(p.readings(), _host_readings(up, dev, [np.asarray(im) for im in im2]))
    got = up(imgs).result()                                          # and the first images give their bytes and texts again
    _same(got[0], images)
    assert got[1] == texts


def test_reader_refusals_and_unchanged_behaviour(dev, gen, crnn):
    from tatt_amd.infer import SuperResolver
    crops = [_img(80 + i, hs, ws) for i, (hs, ws) in enumerate(((16, 64), (23, 90), (9, 40)))]
    with pytest.raises(ValueError, match=r"recognizer=.*long_lines=True"):
        SuperResolver(gen, batch_size=4, lr_size=LR, reader=crnn)(crops)
    with pytest.raises(ValueError, match="recogni"):                 # the recogniser's refusals stay
        SuperResolver(gen, recognizer=crnn, reader=crnn, long_lines=True)
    with pytest.raises(ValueError, match="recogni"):
        SuperResolver(gen, recognizer=crnn, reader=crnn).scene(_img(60, 48, 160, 1), [(0, 0, 64, 16)])
    want_images, want_texts = SuperResolver(gen, batch_size=4, lr_size=LR, recognizer=crnn)(crops).result()
    images, texts = SuperResolver(gen, batch_size=4, lr_size=LR, recognizer=crnn, reader=crnn)(crops).result()
    _same(images, want_images)
    assert texts == want_texts and len(texts) == 3
    with pytest.raises(RuntimeError, match="reader"):
        SuperResolver(gen, batch_size=4, lr_size=LR, long_lines=True)(crops[:1]).readings()
