"""Reading lines of several words against a lexicon on the GPU (csrc/ctcwords.hip; read.ctc_words_read, read.LineReader(decode="words"),
infer.SuperResolver(read_decode="words")).  The yardstick has two stages, so that nothing needs a margin:
(a) the device's log-soft-max `lp_out` against the specification's (read._log_softmax_row in float64) within the project's usual bar,
    measured per case FROM THE SPECIFICATION ALONE: 4 x the largest |float64 - longdouble| of the specification + 2^-52 x max |lp|;
    -inf equal as such;
(b) the specification `read.ctc_words_host` run ON THE DEVICE'S OWN lp_out equals the record BIT FOR BIT: the 64 bits of logp, the
    number of words, every word index, every first and last step, the flag -- on every line of every shape: after the log-soft-max
    there are only float64 additions and comparisons.
Shapes: tests/test_words.py cases() and planted_lines."""
import math
import struct

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests.test_lexicon import ABC, random_words
from tests.test_lines_device_gpu import LR, _generator, _img, _same
from tests.test_read_device_gpu import _upload
from tests.test_words import (ABC27, NEG, brute_force_words, case_inputs, cases, check_planted, degenerate_word_lines, log_softmax_rows,
                              planted_lines, spans_fit)

pytestmark = pytest.mark.gpu
FILL = -77
BITS = lambda v: struct.pack("<d", v)


def _run(dev, x, lex, wp=0.0, index=None, n_rows=None, extra=0):
    """one launch on contiguous logits -> (WordsDecoded per record row, the record on the host, lp_out on the host)"""
    from tatt_amd import read
    T, B, C = x.shape
    rows = B if n_rows is None else n_rows
    rec = torch.full((rows, read.words_record_words(T) + extra), FILL, dtype=torch.int32, device=dev)
    lp = torch.full((B, T, C), 12345.0, dtype=torch.float64, device=dev)
    idx = torch.arange(B, dtype=torch.int32) if index is None else torch.tensor(index, dtype=torch.int32)
    read.ctc_words_read(x.to(dev), lex, idx.to(dev), rec, T, wp, lp)
    return rec.cpu(), lp.cpu()


def _stage_a(x, lp, what):
    """(a): -> (bar, the specification's own distance, the largest |device - specification|) over the clean lines"""
    dist = top = worst = 0.0
    for b in range(x.shape[1]):
        want, wide = log_softmax_rows(x, b), log_softmax_rows(x, b, np.longdouble)
        if any(r is None for r in want):
            continue
        for t, (r, w) in enumerate(zip(want, wide)):
            for c, (v, u) in enumerate(zip(r, w)):
                if v != NEG:
                    dist, top = max(dist, abs(float(np.longdouble(v) - u))), max(top, abs(v))
    bar = 4 * dist + 2.0 ** -52 * top
    for b in range(x.shape[1]):
        want = log_softmax_rows(x, b)
        if any(r is None for r in want):
            assert bool(torch.isnan(lp[b]).all()), (what, b)
            continue
        got = lp[b].tolist()
        for t, (r, g) in enumerate(zip(want, got)):
            for c, (v, u) in enumerate(zip(r, g)):
                if v == NEG:
                    assert u == NEG, (what, b, t, c, u)
                else:
                    assert abs(u - v) <= bar, (what, b, t, c, u, v, bar)
                    worst = max(worst, abs(u - v))
    return bar, dist, worst


def _stage_b(host, lp, lex, wp, T, what, rows=None):
    """(b): every record row equals the specification run on the device's own lp_out, bit for bit -> the decoded rows"""
    from tatt_amd import read
    width = read.words_record_words(T)
    out = []
    for b in range(lp.shape[0]):
        r = b if rows is None else rows[b]
        if r is None:
            continue
        got = read.parse_words_records(host[r:r + 1, :width].contiguous(), T)[0]
        if bool(torch.isnan(lp[b]).any()):
            assert got.flag == 1 and got.words == [] and math.isnan(got.logp) and host[r, 0] == 0, (what, b, got)
            assert bool((host[r, 4:] == FILL).all()), (what, b)
        else:
            want = read.ctc_words_host(lp[b].tolist(), lex, wp)
            assert got.flag == 0 and BITS(got.logp) == BITS(want.logp) and got.words == want.words, (what, b, got, want)
            assert host[r, 0] == len(want.words) and host[r, 1] == 0
            assert bool((host[r, 4 + 2 * len(want.words):] == FILL).all()), (what, b)        # the canary beyond the stated words
        out.append(got)
    return out


@pytest.mark.parametrize("name", ["one-step", "all-6", "reader-T", "every-class", "lane-limit", "both-limits", "penalty-minus",
                                  "penalty-plus"])
def test_the_record_equals_the_specification_on_the_devices_own_log_softmax(dev, name):
    """Measured on an MI355X: see the README, section "Word segmentation" (the bar and the distance of every case)."""
    from tatt_amd import read
    T, n, C, alphabet, words, wp, seed = cases()[name]
    x, lex, wp = case_inputs(name)
    host, lp = _run(dev, x, lex, wp)
    bar, dist, worst = _stage_a(x, lp, name)
    print("case %s (T %d, n %d, C %d, K %d, lanes %d, classes %s, penalty %g): bar %.3g (float64 - longdouble of the specification %.3g), "
          "device - specification of lp %.3g" % (name, T, n, C, len(lex), read.words_lanes(lex), lex.counts, wp, bar, dist, worst))
    got = _stage_b(host, lp, lex, wp, T, name)
    assert len(got) == n
    print("case %s: words per line %s: bit-equal" % (name, [len(g.words) for g in got]))
    if name == "all-6":                                              # every string of length <= 2, also against brute force
        for b, g in enumerate(got):
            best, paths = brute_force_words(lp[b].tolist(), lex)
            assert BITS(g.logp) == BITS(best) and any(spans_fit(g, lex, p) for p in paths)
    if name == "lane-limit":
        assert read.words_lanes(lex) == read.words_limits()["lanes"]
    if name in ("reader-T", "every-class", "lane-limit"):
        assert any(len(g.words) >= 2 for g in got)


def test_planted_lines_on_the_device(dev):
    x, planted, lex = planted_lines(range(17))
    host, lp = _run(dev, x, lex)
    bar, dist, worst = _stage_a(x, lp, "planted")
    print("planted lines (T 64, n 17, C 27, K 9): bar %.3g (float64 - longdouble %.3g), device - specification of lp %.3g" % (bar, dist, worst))
    got = _stage_b(host, lp, lex, 0.0, 64, "planted")
    for g, (string, runs) in zip(got, planted):
        check_planted(g, lex, string, runs)


def test_every_comparison_a_tie(dev):
    """all logits equal: the order of the list and of the classes decides everything, as the specification states it"""
    from tatt_amd import read
    for words in (["to", "day", "today", "a", "y"], ["today", "y", "to", "a", "day"]):
        lex = read.Lexicon(words, alphabet=ABC27)
        x = torch.zeros(9, 2, 27)
        host, lp = _run(dev, x, lex)
        _stage_a(x, lp, "ties")
        got = _stage_b(host, lp, lex, 0.0, 9, "ties")
        assert got[0] == got[1] and got[0].flag == 0


def test_flagged_and_degenerate_lines_beside_clean_ones_and_the_index(dev):
    from tatt_amd import read
    x, lex, flags = degenerate_word_lines()
    T, B = x.shape[0], x.shape[1]
    host, lp = _run(dev, x, lex, extra=5)
    _stage_a(x, lp, "degenerate")
    got = _stage_b(host, lp, lex, 0.0, T, "degenerate")
    assert [g.flag for g in got] == flags
    assert got[4].words and got[4].logp > NEG and got[5] == read.WordsDecoded([], NEG, 0)
    # scattered rows in a larger record, two lines sent nowhere
    n_rows = B + 3
    order = [n_rows - 1 - b for b in range(B)]
    order[1], order[4] = -1, n_rows
    host2, lp2 = _run(dev, x, lex, index=order, n_rows=n_rows, extra=5)
    for r in range(n_rows):
        if r not in order:
            assert bool((host2[r] == FILL).all()), r                 # untouched rows keep their fill
    for b in (1, 4):
        assert bool((lp2[b] == 12345.0).all())                       # a line without a row writes nothing at all
    again = _stage_b(host2, torch.where(lp2 == 12345.0, lp, lp2), lex, 0.0, T, "scattered", rows=[r if 0 <= r < n_rows else None for r in order])
    key = lambda g: (g.words, g.flag, BITS(g.logp))
    assert [key(g) for g in again] == [key(g) for b, g in enumerate(got) if b not in (1, 4)]
    rec = torch.full((2, read.words_record_words(T)), FILL, dtype=torch.int32, device=dev)
    read.ctc_words_read(x.to(dev), lex, torch.tensor([-1, 2, -5, 2 ** 30, 7, 9], dtype=torch.int32).to(dev), rec, T)
    torch.cuda.synchronize()
    assert bool((rec == FILL).all())                                 # no index inside 0 .. n_rows - 1: nothing is written


def test_refusals_before_any_launch(dev):
    from tatt_amd import read
    lanes = read.words_limits()["lanes"]
    over = read.Lexicon(["%d" % i for i in range(10 ** 6, 10 ** 6 + lanes // 16 + 1)])
    assert read.words_lanes(over) > lanes
    x = torch.zeros(4, 1, 37, device=dev)
    rec = torch.full((1, read.words_record_words(4)), FILL, dtype=torch.int32, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="lanes"):
        read.ctc_words_read(x, over, idx, rec, 4)
    lex = read.Lexicon(["ab"])
    with pytest.raises(ValueError, match="word_penalty"):
        read.ctc_words_read(x, lex, idx, rec, 4, math.inf)
    with pytest.raises(ValueError):
        read.ctc_words_read(x, lex, idx, rec[:, :-1], 4)
    with pytest.raises(ValueError):
        read.ctc_words_read(x, lex, idx, rec, 3)                     # cap < T
    with pytest.raises(ValueError):
        read.ctc_words_read(x, lex, idx, rec, 4, 0.0, torch.zeros(1, 4, 36, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        read.ctc_words_read(x, read.Lexicon(["a"], alphabet=ABC + "!"), idx, rec, 4)
    torch.cuda.synchronize()
    assert bool((rec == FILL).all())
    read.ctc_words_read(x, lex, idx, rec, 4)                         # lp_out is optional
    assert read.parse_words_records(rec.cpu(), 4)[0].flag == 0


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
SOURCES = ((16, 64), (16, 72), (16, 76))                             # rw 100, 120, 120: a bucket of one line and a bucket of two
WORDS = random_words(ABC, 24, (1, 2, 3, 4, 5, 8), 71)


@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


def test_line_reader_reads_words(dev, crnn):
    """every WordsReading equals the specification run on the reader's own kept lp_out, bit for bit, with the spans in pixels"""
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    images = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result()
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    lex = read.Lexicon(WORDS)
    for wp in (0.0, -1.5):
        reader = read.LineReader(crnn, batch_size=8, keep_logits=True, decode="words", lexicon=lex, word_penalty=wp, keep_lp=True)
        assert reader.lexicon is lex and reader.word_penalty == wp
        launches, real = [], read.ctc_words_read

        def counted(*a):
            launches.append(a[0].shape)
            return real(*a)
        read.ctc_words_read = counted
        try:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")                  # nothing waits for the device before result()
            try:
                pending = reader.read(buf, rows, 2)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        finally:
            read.ctc_words_read = real
        assert [tuple(s) for s in launches] == [(26, 1, 37), (31, 2, 37)]      # one launch per bucket chunk
        readings = pending.result()
        assert [idx for idx, _ in pending.logits] == [idx for idx, _ in pending.lp] == [[0], [1, 2]]
        assert [(r.rw, r.squeezed) for r in readings] == [(100, False), (120, False), (120, False)]
        assert pending.texts() == [r.text for r in readings] and all(isinstance(r, read.WordsReading) for r in readings)
        for (idx, lg), (_, lp) in zip(pending.logits, pending.lp):
            assert tuple(lp.shape) == (len(idx), lg.shape[0], 37) and lp.dtype == torch.float64
            bar, dist, worst = _stage_a(lg.cpu(), lp.cpu(), "reader")
            for j, i in enumerate(idx):
                want = read.ctc_words_host(lp[j].cpu().tolist(), lex, wp)
                r, W = readings[i], rows[i][2]
                print("line %d (penalty %g): bar %.3g, device - specification of lp %.3g, words %r" % (i, wp, bar, worst, r.text))
                assert BITS(r.logp) == BITS(want.logp) and [(s.index, s.first, s.last) for s in r.words] == want.words
                assert r.text == " ".join(lex.words[k] for k, _, _ in want.words) and all(s.text == lex.words[s.index] for s in r.words)
                assert [(s.x0, s.x1) for s in r.words] == [read.word_span_pixels(f, l, W, r.rw) for _, f, l in want.words]
                assert all(0 <= s.x0 < s.x1 <= W for s in r.words)
    assert not reader.read(buf, [], 2).result() and read.LineReader(crnn, decode="words", lexicon=lex).read(buf, rows, 2).lp is None


def test_super_resolver_reads_words(dev, crnn):
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    from tests.test_quads_device_gpu import QUADS
    from tests.test_scene_device_gpu import BOXES
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    up = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_decode="words", read_lexicon=WORDS,
                       read_word_penalty=-0.5)
    assert (up.reader.decode, up.reader.word_penalty, up.reader.lexicon.words) == ("words", -0.5, WORDS)
    p = up(imgs)
    images, texts = p.result()
    _same(images, SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result())
    rs = p.readings()
    assert texts == [r.text for r in rs] and len(texts) == 3 and all(isinstance(r, read.WordsReading) for r in rs)
    assert all(all(w in WORDS for w in t.split(" ")) for t in texts if t)
    assert [(r.rw, r.squeezed) for r in rs] == [(100, False), (120, False), (120, False)]
    lex = read.Lexicon(WORDS, min_segment=64)
    scene_up = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn, read_decode="words", read_lexicon=lex)
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32)
    for scene, regions, run, run_plain in ((_img(60, 48, 160, 1), BOXES, scene_up.scene, plain.scene),
                                           (_img(61, 97, 211, 1), QUADS, scene_up.scene_quads, plain.scene_quads)):
        q = run(scene, regions, 2)
        _same([q.result()], [run_plain(scene, regions, 2).result()])
        rs = q.readings()
        assert len(rs) == len(regions) and q.texts() == [r.text for r in rs]
        assert all(isinstance(r, read.WordsReading) and not math.isnan(r.logp) and r.text == " ".join(s.text for s in r.words) for r in rs)
    with pytest.raises(ValueError, match="lexicon="):
        SuperResolver(gen, reader=crnn, read_decode="words")
    with pytest.raises(ValueError, match="word_penalty"):
        SuperResolver(gen, reader=crnn, read_decode="greedy", read_word_penalty=-1.0)


def test_the_other_decodings_enqueue_what_they_enqueued(dev, crnn):
    """without the new keyword a call makes no words launch and the same library calls through ops.call in the same order"""
    from tatt_amd import ops, read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    images = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)([_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]).result()
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    seen, real_call, real_words = {}, ops.call, read.ctc_words_read
    for decode, kw in (("greedy", {}), ("beam", {"beam": 8, "nbest": 4}), ("lexicon", {"lexicon": WORDS}), ("words", {"lexicon": WORDS})):
        reader = read.LineReader(crnn, batch_size=8, decode=decode, **kw)
        reader.read(buf, rows, 2).result()                           # (folds and packs are made)
        calls, words = [], []
        ops.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        read.ctc_words_read = lambda *a: (words.append(1), real_words(*a))[1]
        try:
            reader.read(buf, rows, 2).result()
        finally:
            ops.call, read.ctc_words_read = real_call, real_words
        seen[decode] = (calls, len(words))
    assert [seen[d][1] for d in ("greedy", "beam", "lexicon", "words")] == [0, 0, 0, 2]
    forward = [c for c in seen["greedy"][0] if c != "tatt_ctc_greedy_read"]
    assert seen["greedy"][0].count("tatt_ctc_greedy_read") == 2 and len(forward) >= 2
    assert seen["beam"][0] == forward and seen["lexicon"][0] == forward and seen["words"][0] == forward
