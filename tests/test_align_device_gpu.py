"""CTC forced alignment on the GPU (csrc/ctcalign.hip; read.ctc_align, read.LineReader(locate=True), read.LineReader.align,
infer.SuperResolver(read_locate=True)).  The yardstick has two stages, so that nothing needs a margin:
(a) the device's log-soft-max `lp_out` against the specification's (read._log_softmax_row in float64) within the project's usual bar,
    measured per case FROM THE SPECIFICATION ALONE: 4 x the largest |float64 - longdouble| of the specification + 2^-52 x max |lp|;
    -inf equal as such;
(b) the specification `read.ctc_align_host` run ON THE DEVICE'S OWN lp_out equals the record BIT FOR BIT: n, the flag, the 64 bits of
    logp, every (first, last), the 64 bits of every char_logp, and every other word of every row (the canary behind the stated
    characters, the decode part a string was read from, rows without a line) as it was -- on every line of every launch: after the
    log-soft-max there are only float64 additions and comparisons.
The launches are tests/test_align.py `launches()` (tools/align_host_check.py runs the same ones off the GPU).
Measured on an MI355X: see the README, section "Locating what was read" (the bar and the distance of every launch)."""
import math

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests.test_align import BITS, FILL, LP_FILL, NEG, brute_force, launches, stage_a, stage_b
from tests.test_lines_device_gpu import LR, _generator, _img, _same
from tests.test_read_device_gpu import _upload
from tests.test_words_device_gpu import SOURCES

pytestmark = pytest.mark.gpu
LAUNCHES = {l["name"]: l for l in launches()}


def _run(dev, l):
    """one launch -> (the record after it on the host, lp_out on the host)"""
    from tatt_amd import read
    x = l["x"]
    T, B, C = x.shape
    xd = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=dev) if not x.is_contiguous() else None
    if xd is None:
        xd = x.to(dev)
    else:
        xd.copy_(x)
        assert xd.stride() == x.stride() and not xd.is_contiguous()
    rec = l["before"].to(dev)
    src = rec if l["table"] is None else l["table"].to(dev)
    lp = torch.full((B, T, C), LP_FILL, dtype=torch.float64, device=dev)
    read.ctc_align(xd, torch.tensor(l["index"], dtype=torch.int32).to(dev), src, l["len_at"], l["cls_at"], l["gate_at"], rec, l["rec_at"],
                   l["cap_len"], lp)
    return rec.cpu(), lp.cpu()


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_the_record_equals_the_specification_on_the_devices_own_log_softmax(dev, name):
    l = LAUNCHES[name]
    x = l["x"]
    T, B, C = x.shape
    after, lp = _run(dev, l)
    bar, dist, worst = stage_a(x, lp, l["index"], l["before"].shape[0], name)
    print("launch %s (T %d, n %d, C %d, cap_len %d): bar %.3g (float64 - longdouble of the specification %.3g), device - specification "
          "of lp %.3g" % (name, T, B, C, l["cap_len"], bar, dist, worst))
    got = stage_b(lp, l["sources"], l["index"], l["before"], after, l["rec_at"], l["cap_len"], C, name)
    assert len(got) == B
    print("launch %s: flags %s, characters %s: bit-equal" % (name, "".join("-" if g is None else str(g.flag) for g in got),
                                                              [None if g is None else len(g.spans) for g in got]))
    flags = [None if g is None else g.flag for g in got]
    if name.startswith("all-15"):                                    # every string of length <= 3 over two characters: brute force too
        for b, g in enumerate(got):
            want = brute_force(lp[b].tolist()).get(tuple(l["sources"][b][1]), NEG)
            assert BITS(g.logp) == BITS(want), (b, g, want)
        by = {tuple(s[1]): g for s, g in zip(l["sources"], got)}
        assert all(by[k].logp == NEG and by[k].spans == [] for k in ((1, 1, 1), (2, 2, 2)) if k in by)
        assert all(by[k].spans == [(0, 0), (2, 2)] for k in ((1, 1), (2, 2)) if k in by)
    if name == "limit":
        assert all(len(g.spans) == 127 and g.logp > NEG for g in got)
    if name.startswith("wave-edge"):
        assert [len(g.spans) for g in got[:3]] == [31, 32, 33] and len(got[14].spans) == 64       # 63 / 65 / 67 states: astride a wave
    if name.startswith("reader-T"):
        assert [len(g.spans) for g in got] == [0, 7, 26] and got[2].spans == [(t, t) for t in range(26)]
    if name == "refused":
        assert flags == [0, 2, 2, 2, 2, 0]
    if name == "over-cap":
        assert flags == [0, 2, 0, 0, 0, 0]
    if name == "degenerate":
        assert flags == [0, 1, 1, 1, 1, 0]
    if name == "scattered":
        assert flags == [0, None, 0, 1, None, 0]
    if name == "ties":
        assert got[1].spans == [(0, 0), (1, 1), (2, 2)] and got[2].spans == [(0, 0), (2, 2), (3, 3)] and len(got[3].spans) == 8


def test_refusals_before_any_launch(dev):
    from tatt_amd import read
    x = torch.zeros(4, 1, 37, device=dev)
    rec = torch.full((1, read.align_record_words(4) + 2), FILL, dtype=torch.int32, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    src = torch.from_numpy(read.pack_strings([[1, 2]], 4)).to(dev)
    with pytest.raises(ValueError):
        read.ctc_align(torch.zeros(257, 1, 37, device=dev), idx, src, 0, 2, -1, rec, 0, 4)            # T beyond the limit
    with pytest.raises(ValueError):
        read.ctc_align(torch.zeros(4, 1, 65, device=dev), idx, src, 0, 2, -1, rec, 0, 4)              # C beyond the limit
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, torch.zeros(1, 130, dtype=torch.int32, device=dev), 0, 2, -1,
                       torch.zeros(1, read.align_record_words(128), dtype=torch.int32, device=dev), 0, 128)   # cap_len beyond it
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 0, 2, -1, rec, 1, 4)                                               # an odd rec_at
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 0, 2, -1, rec, 4, 4)                                               # the part leaves the row
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 0, 2, -1, torch.full((1, 21), FILL, dtype=torch.int32, device=dev), 0, 4)   # an odd stride
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 0, 3, -1, rec, 0, 4)                                               # the classes leave the source row
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 6, 2, -1, rec, 0, 4)
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 0, 2, 6, rec, 0, 4)
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src.to(torch.int64), 0, 2, -1, rec, 0, 4)
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src, 0, 2, -1, rec, 0, 4, torch.zeros(1, 4, 36, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        read.ctc_align(x, idx, src[:0], 0, 2, -1, rec, 0, 4)                                           # fewer source rows than record rows
    torch.cuda.synchronize()
    assert bool((rec == FILL).all())                                 # the record still all fill
    read.ctc_align(x, idx, src, 0, 2, -1, rec, 2, 4)                 # lp_out is optional
    got = read.parse_align_records(rec.cpu()[:, 2:], 4)[0]
    assert got.flag == 0 and got.spans == [(0, 0), (1, 1)] and bool((rec.cpu()[0, :2] == FILL).all())


# ---- the reader -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


@pytest.fixture(scope="module")
def lines(dev):
    from tatt_amd.infer import SuperResolver
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    images = SuperResolver(_generator(dev), batch_size=8, lr_size=LR, long_lines=True)(imgs).result()
    return _upload(dev, [np.asarray(im) for im in images])


def _counted(fn):
    """fn() with read.ctc_align counted and no host wait allowed -> (what fn returned, the logits shapes of the align launches)"""
    from tatt_amd import read
    launches_, real = [], read.ctc_align

    def counted(*a):
        launches_.append(tuple(a[0].shape))
        return real(*a)
    read.ctc_align = counted
    try:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                      # nothing waits for the device before result()
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        read.ctc_align = real
    return out, launches_


def _check_locations(read, locs, pending, rows, alphabet, texts):
    """every LineLocation equals the specification run on the reader's own kept lp with the given string, bit for bit"""
    a2d = {ch: i for i, ch in enumerate(alphabet)}
    assert [idx for idx, _ in pending.logits] == [idx for idx, _ in pending.lp] == [[0], [1, 2]]
    for (idx, lg), (_, lp) in zip(pending.logits, pending.lp):
        assert tuple(lp.shape) == (len(idx), lg.shape[0], 37) and lp.dtype == torch.float64
        bar, dist, worst = stage_a(lg.cpu(), lp.cpu(), list(range(len(idx))), len(idx), "reader")
        for j, i in enumerate(idx):
            loc, W = locs[i], rows[i][2]
            assert loc.text == texts[i] and (loc.rw, loc.squeezed) == ((100, 120, 120)[i], False)
            classes = [a2d[ch] for ch in loc.text]
            want = read.ctc_align_host(lp[j].cpu().tolist(), classes)
            print("line %d: bar %.3g, device - specification of lp %.3g, %d characters, logp %.17g" % (i, bar, worst, len(classes), loc.logp))
            assert loc.flag == 0 and BITS(loc.logp) == BITS(want.logp) and len(loc.chars) == len(want.spans)
            assert [(c.first, c.last) for c in loc.chars] == want.spans and [BITS(c.logp) for c in loc.chars] == [BITS(v) for v in want.char_logp]
            assert [(c.char, c.cls) for c in loc.chars] == [(ch, a2d[ch]) for ch in loc.text[:len(loc.chars)]]
            assert [(c.x0, c.x1) for c in loc.chars] == [read.word_span_pixels(f, l, W, loc.rw) for f, l in want.spans]
            assert all(0 <= c.x0 < c.x1 <= W for c in loc.chars)


@pytest.mark.parametrize("decode", ["greedy", "beam", "beam-lm", "beam-pattern"])
def test_line_reader_locates_what_it_reads(dev, crnn, lines, decode):
    from tatt_amd import read
    buf, rows = lines
    kw = {"decode": "greedy" if decode == "greedy" else "beam"}
    if decode == "beam-lm":
        kw["lm"] = read.CharLM.from_corpus(["abc", "a1b2", "zebra 9".replace(" ", "")], order=2)
    if decode == "beam-pattern":
        kw["pattern"] = ".*"
    reader = read.LineReader(crnn, batch_size=8, keep_logits=True, keep_lp=True, locate=True, **kw)
    assert reader.locate
    pending, counted = _counted(lambda: reader.read(buf, rows, 2))
    assert counted == [(26, 1, 37), (31, 2, 37)]                     # one align launch per bucket chunk
    readings, locs = pending.result(), pending.locations()
    assert len(locs) == 3 and all(isinstance(l, read.LineLocation) for l in locs)
    assert pending.texts() == [r.text for r in readings]
    _check_locations(read, locs, pending, rows, read._alphabet(), pending.texts())
    plain = read.LineReader(crnn, batch_size=8, **kw).read(buf, rows, 2)
    assert plain.result() == readings and plain.lp is None           # the readings are those without the keyword
    with pytest.raises(ValueError, match="locate"):
        plain.locations()
    if decode == "greedy":
        assert any(r.text for r in readings)
        for r, l in zip(readings, locs):                             # tie-free logits: a greedy run begins where its character is entered
            assert [c.first for c in l.chars] == r.steps and [c.cls for c in l.chars] == r.chars
        # aligning the greedy texts as KNOWN strings reproduces the locations: no decode launch, one align launch per chunk
        from tatt_amd import ops
        calls, real_call = [], ops.call
        ops.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        try:
            again, counted = _counted(lambda: reader.align(buf, rows, 2, pending.texts()))
        finally:
            ops.call = real_call
        assert counted == [(26, 1, 37), (31, 2, 37)] and "tatt_ctc_greedy_read" not in calls
        assert isinstance(again, read.PendingAlignment) and again.locations() == locs
        _check_locations(read, again.locations(), again, rows, read._alphabet(), pending.texts())
        with pytest.raises(ValueError, match="line 1"):
            reader.align(buf, rows, 2, ["ab", "a!", "c"])
        with pytest.raises(ValueError, match="line 2"):
            reader.align(buf, rows, 2, ["ab", "a", "c" * 128])
        with pytest.raises(ValueError):
            reader.align(buf, rows, 2, ["ab"])
        assert reader.align(buf, [], 2, []).locations() == [] and reader.read(buf, [], 2).locations() == []
        hard = reader.align(buf, rows, 2, ["", "zz", "q" * 40]).locations()         # "q" * 40 needs 79 steps: the line has 31
        assert hard[0].chars == [] and hard[0].logp > NEG and len(hard[1].chars) == 2 and hard[2].logp == NEG and hard[2].chars == []
        assert hard[2].text == "q" * 40 and hard[2].flag == 0


def test_locate_goes_with_greedy_and_beam_only(dev, crnn):
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    for decode, kw in (("lexicon", {"lexicon": ["ab"]}), ("words", {"lexicon": ["ab"]}), ("lexicons", {})):
        with pytest.raises(ValueError, match="locate"):
            read.LineReader(crnn, decode=decode, locate=True, **kw)
    with pytest.raises(ValueError, match="read_locate"):
        SuperResolver(_generator(dev), read_locate=True)


# ---- through the scene paths ----------------------------------------------------------------------------------------------------------
def _inside(region, scale, pt, eps=1e-9):
    """whether pt lies within the region's outline (times scale), up to eps: in one of its convex parts"""
    from tatt_amd import locate
    from tatt_amd.polys import poly_strips
    kind = locate.region_kind(region)
    if kind == "box":
        x0, y0, x1, y1 = region
        parts = [((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    else:
        parts = [tuple(region)] if kind == "quad" else poly_strips(tuple(region))
    for part in parts:
        ok = True
        for a, b in zip(part, part[1:] + part[:1]):
            ax, ay, bx, by = scale * a[0], scale * a[1], scale * b[0], scale * b[1]
            cross = (bx - ax) * (pt[1] - ay) - (by - ay) * (pt[0] - ax)              # >= 0 inside a clockwise part (y down)
            ok = ok and cross / math.hypot(bx - ax, by - ay) >= -eps
        if ok:
            return True
    return False


def test_super_resolver_locates_in_the_picture(dev, crnn):
    from tatt_amd import locate, read
    from tatt_amd.infer import SuperResolver
    from tests.test_polys_device_gpu import POLYS
    from tests.test_quads_device_gpu import QUADS
    from tests.test_scene_device_gpu import BOXES
    gen = _generator(dev)
    up = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn, read_locate=True)
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32)
    assert up.reader.locate and up.reader.decode == "greedy"
    some = 0
    for scene, regions, run, run_plain in ((_img(60, 48, 160, 1), BOXES, up.scene, plain.scene),
                                           (_img(61, 97, 211, 1), QUADS, up.scene_quads, plain.scene_quads),
                                           (_img(60, 96, 200, 1), POLYS, up.scene_polys, plain.scene_polys)):
        q = run(scene, regions, 2)
        _same([q.result()], [run_plain(scene, regions, 2).result()])   # the picture is the one without the keyword
        locs, inner = q.locations(), q._reading.locations()
        assert len(locs) == len(regions) and q.texts() == [l.text for l in locs]
        widths = [int(w) for w in q._reading._plan.desc[:, 2]]
        for l, plain_l, region, W in zip(locs, inner, regions, widths):
            assert l._replace(chars=None) == plain_l._replace(chars=None) and len(l.chars) == len(plain_l.chars)
            for c, p in zip(l.chars, plain_l.chars):
                some += 1
                assert isinstance(c, locate.LocatedChar) and c[:7] == tuple(p)
                assert c.polygon == locate.span_polygon(region, W, p.x0, p.x1, 2) and len(c.polygon) >= 4
                assert all(_inside(region, 2, pt) for pt in c.polygon), (region, c)
    assert some > 0
    # long_lines: the rectangle in the returned image, scaled by out_sizes where given
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    for out_sizes in (None, [(90, 20), (200, 32), (77, 31)]):
        lp_ = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_locate=True)(imgs, out_sizes=out_sizes)
        images, texts = lp_.result()
        _same(images, SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs, out_sizes=out_sizes).result())
        locs = lp_.locations()
        assert [l.text for l in locs] == texts and len(locs) == 3
        for l, im, W in zip(locs, images, [int(w) for w in lp_._reading._plan.desc[:, 2]]):
            for c in l.chars:
                assert c.polygon == locate.line_polygon(32, W, c.x0, c.x1, None if out_sizes is None else im.size)
                assert all(0 <= x <= im.size[0] and 0 <= y <= im.size[1] for x, y in c.polygon)


def test_without_the_keyword_every_decoding_enqueues_what_it_enqueued(dev, crnn, lines):
    """the same ops.call sequence with and without locate= (the align launch is no ops.call), and no align launch without it"""
    from tatt_amd import ops, read
    buf, rows = lines
    real_call, real_align = ops.call, read.ctc_align
    lm = read.CharLM.from_corpus(["abc", "a1b2"], order=2)
    for decode, kw in (("greedy", {}), ("beam", {"beam": 8, "nbest": 4}), ("beam", {"lm": lm}), ("beam", {"pattern": ".*"}),
                       ("lexicon", {"lexicon": ["ab", "b"]}), ("words", {"lexicon": ["ab", "b"]})):
        seen = []
        for locate_kw in ({}, {"locate": True}):
            if locate_kw and decode not in ("greedy", "beam"):
                continue
            reader = read.LineReader(crnn, batch_size=8, decode=decode, **kw, **locate_kw)
            reader.read(buf, rows, 2).result()                       # (folds and packs are made)
            calls, aligns = [], []
            ops.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
            read.ctc_align = lambda *a: (aligns.append(1), real_align(*a))[1]
            try:
                reader.read(buf, rows, 2).result()
            finally:
                ops.call, read.ctc_align = real_call, real_align
            seen.append((calls, len(aligns)))
        assert seen[0][1] == 0 and len(seen[0][0]) >= 2, (decode, kw)
        if len(seen) == 2:
            assert seen[1] == (seen[0][0], 2), (decode, kw)
