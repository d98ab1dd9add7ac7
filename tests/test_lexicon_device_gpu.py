"""Reading lines against a lexicon on the GPU (csrc/ctclex.hip; read.ctc_lexicon_score, read.ctc_lexicon_select,
read.LineReader(decode="lexicon"), infer.SuperResolver(read_decode="lexicon")).  Yardstick: the host specification
read.ctc_lexicon_scores_host / ctc_lexicon_read_host in float64, itself held to brute force by tests/test_lexicon.py.  Every finite score
of every word and line within a bar that is measured per case FROM THE SPECIFICATION ALONE: 4 x the distance of the float64 specification
from the same specification run in np.longdouble, plus T x 2^-52 x max |score| (one rounding of the running sum per step); -inf and NaN
equal as such; logz within that plus K x 2^-52 (the device sums K terms, each at most 1, in another order).  The ORDER of a line's entries
is compared on every line, behind margin > 100 x bar, and no line may be left out.  Shapes: tests/test_lexicon.py CASES."""
import math
import random

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests.test_beam import beam_logits, brute_force
from tests.test_lexicon import ABC, CASES, TIES, case_lexicon, degenerate_lines, lexicon_case, random_words, spec_bar
from tests.test_lines_device_gpu import LR, _generator, _img, _same
from tests.test_read_device_gpu import _upload

pytestmark = pytest.mark.gpu
FILL = -77


def _run(dev, x, lex, nbest):
    """the launches on contiguous logits, rows in input order -> ((B, K) float64 scores, LexiconDecoded per line, the record), on the host"""
    from tatt_amd import read
    B = x.shape[1]
    scores = torch.full((B, len(lex)), 12345.0, dtype=torch.float64, device=dev)
    rec = torch.full((B, read.lexicon_record_words(nbest)), FILL, dtype=torch.int32, device=dev)
    read.ctc_lexicon_score(x.to(dev), lex, scores)
    read.ctc_lexicon_select(scores, torch.arange(B, dtype=torch.int32).to(dev), rec, nbest)
    host = rec.cpu()
    return scores.cpu(), read.parse_lexicon_records(host, nbest), host


def _compare_scores(got, want, bar, what):
    """got: (B, K) tensor, want: the specification's lists (None: a flagged line) -> the largest |device - specification| of a finite score"""
    worst = 0.0
    for b, row in enumerate(want):
        g = got[b].tolist()
        for k, v in enumerate(g):
            if row is None:
                assert math.isnan(v), (what, b, k, v)
            elif row[k] == -math.inf:
                assert v == -math.inf, (what, b, k, v)
            else:
                assert abs(v - row[k]) <= bar, (what, b, k, v, row[k], bar)
                worst = max(worst, abs(v - row[k]))
    return worst


def _host_topk(row, nbest):
    """the device's OWN scores of a line -> its entries: exact, whatever the scores are"""
    finite = sorted((k for k, v in enumerate(row) if v == v and abs(v) != math.inf), key=lambda k: (-row[k], k))
    return [(k, row[k]) for k in finite[:nbest]]


def _compare_decoded(got, dec, scores, host, bar, nbest, what):
    K = scores.shape[1]
    for b, (g, w) in enumerate(zip(got, dec)):
        assert w.margin > 100 * bar, "%s line %d: margin %.3g against a bar of %.3g: take another seed" % (what, b, w.margin, bar)
        assert g.flag == w.flag == 0 and [k for k, _ in g.entries] == [k for k, _ in w.entries], (what, b, g.entries, w.entries)
        assert g.entries == _host_topk(scores[b].tolist(), nbest)    # the entries carry the score buffer's float64 values as they are
        if w.logz == -math.inf:
            assert g.logz == -math.inf
        else:
            assert abs(g.logz - w.logz) <= bar + K * 2.0 ** -52, (what, b, g.logz, w.logz)
        n = len(g.entries)
        assert host[b, 0] == n and host[b, 1] == 0 and all(int(host[b, 7 + 4 * i]) == 0 for i in range(n))
        assert bool((host[b, 4 + 4 * n:] == FILL).all())             # words of entries that do not exist are not written


@pytest.mark.parametrize("name", list(CASES))
def test_scores_and_entries_equal_the_specification(dev, name):
    """Measured on an MI355X: see the README, section "Reading lines" (the bar and the distance of every case)."""
    T, n, C, alphabet, words, nbest, seed = CASES[name]
    x, lex, want, dec, bar, dist = lexicon_case(name)
    scores, got, host = _run(dev, x, lex, nbest)
    worst = _compare_scores(scores, want, bar, name)
    print("case %s (T %d, n %d, C %d, K %d, nbest %d, classes %s): bar %.3g (float64 - longdouble of the specification %.3g), "
          "device - specification %.3g, smallest neighbour gap %.3g" % (name, T, n, C, len(lex), nbest, lex.counts, bar, dist, worst,
                                                                       min(d.margin for d in dec)))
    _compare_decoded(got, dec, scores, host, bar, nbest, name)
    if name == "all-15":                                             # every string there is, against brute force over the 27 alignments
        for b in range(n):
            exact = brute_force(x[:, b])
            for k, w in enumerate(lex.classes):
                v = float(scores[b, k])
                assert (v == -math.inf) if tuple(w) not in exact else abs(v - exact[tuple(w)]) <= 1e-14 + bar, (b, w, v)
            assert abs(got[b].logz - math.log(math.fsum(math.exp(v) for v in exact.values()))) <= 1e-14 + bar + 15 * 2.0 ** -52


def test_the_arithmetic_of_a_word_does_not_depend_on_its_segment(dev):
    """the every-class lexicon packed with min_segment = 64 (and 32): the same float64 values bit for bit as packed with 16"""
    name = "every-class"
    x, lex, want, dec, bar, dist = lexicon_case(name)
    nbest = CASES[name][5]
    packed, got, _ = _run(dev, x, lex, nbest)
    for seg in (64, 32):
        wide = case_lexicon(name, min_segment=seg)
        assert wide.words == lex.words and wide.counts != lex.counts and wide.counts[0] == 0
        scores, same, _ = _run(dev, x, wide, nbest)
        assert torch.equal(scores.view(torch.int64), packed.view(torch.int64)), seg
        assert same == got


def test_position_independence_at_a_grid_of_many_tiles(dev):
    from tatt_amd import read
    K, T, n, nbest = 4099, 26, 2, 16
    words = random_words(ABC, K, tuple(range(1, 21)), 31)
    big = read.Lexicon(words)
    assert all(c > 256 for c in big.counts)                          # every class fills many work-groups
    x = beam_logits(T, n, 37, 3.0, 32)
    scores, got, host = _run(dev, x, big, nbest)
    pick = random.Random(33).sample(range(K), 32)
    small = read.Lexicon([words[k] for k in pick])
    assert all(c > 0 for c in small.counts)
    few, _, _ = _run(dev, x, small, 4)
    assert torch.equal(few.view(torch.int64), scores[:, pick].contiguous().view(torch.int64))
    want, bar, dist = spec_bar(x, small)
    worst = _compare_scores(few, want, bar, "sampled words")
    print("K %d, classes %s: 32 sampled words: bar %.3g (float64 - longdouble %.3g), device - specification %.3g" % (K, big.counts, bar,
                                                                                                                    dist, worst))
    assert not bool(torch.isnan(scores).any()) and not bool((scores == 12345.0).any())
    for b in range(n):
        assert got[b].entries == _host_topk(scores[b].tolist(), nbest) and len(got[b].entries) == nbest and got[b].flag == 0
        row = [v for v in scores[b].tolist() if v != -math.inf]
        m = max(row)
        assert abs(got[b].logz - (m + math.log(math.fsum(math.exp(v - m) for v in row)))) <= K * 2.0 ** -52 + 2.0 ** -52 * abs(m)


def test_exact_ties_go_to_the_lower_word_index(dev):
    """all logits equal, six words of length 4 without adjacent repeats: every word goes through the same operations on the same values"""
    from tatt_amd import read
    lex = read.Lexicon(TIES, alphabet="-abcd")
    x = torch.zeros(9, 2, 5)
    spec, bar, _ = spec_bar(x, lex)
    want = read.ctc_lexicon_read_host(x, lex, nbest=6, scores=spec)
    scores, got, _ = _run(dev, x, lex, 6)
    _compare_scores(scores, spec, bar, "ties")
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(set(scores[b].tolist())) == 1
        assert [k for k, _ in g.entries] == [k for k, _ in w.entries] == [0, 1, 2, 3, 4, 5]
        assert abs(g.logz - w.logz) <= bar + len(lex) * 2.0 ** -52
    _, short, _ = _run(dev, x, lex, 3)
    assert [k for k, _ in short[0].entries] == [0, 1, 2] and short[0].logz == got[0].logz


def test_flagged_and_degenerate_lines_beside_clean_ones(dev):
    from tatt_amd import read
    x, lex, flags = degenerate_lines()
    want, bar, dist = spec_bar(x, lex)                               # (the clean lines' scores make the bar; flagged lines have none)
    dec = read.ctc_lexicon_read_host(x, lex, nbest=4, scores=want)
    assert [d.flag for d in dec] == flags and [len(d.entries) for d in dec] == [4, 0, 0, 0, 4, 0]
    scores, got, host = _run(dev, x, lex, 4)
    worst = _compare_scores(scores, want, bar, "degenerate")
    print("degenerate lines: bar %.3g (float64 - longdouble %.3g), device - specification %.3g" % (bar, dist, worst))
    for b, (g, w) in enumerate(zip(got, dec)):
        assert g.flag == w.flag and [k for k, _ in g.entries] == [k for k, _ in w.entries], (b, g, w)
        if w.flag:
            assert math.isnan(g.logz) and host[b, 0] == 0 and host[b, 1] == 1 and bool((host[b, 4:] == FILL).all())
        elif not w.entries:                                          # no word of the lexicon has an alignment: not a flagged line
            assert g.logz == -math.inf and bool((scores[b] == -math.inf).all()) and bool((host[b, 4:] == FILL).all())
        else:
            assert abs(g.logz - w.logz) <= bar + len(lex) * 2.0 ** -52


def test_strided_logits_and_scattered_rows(dev):
    from tatt_amd import read
    name = "reader-T"
    T, B, C, _, _, nbest, _ = CASES[name]
    x, lex, want, dec, bar, dist = lexicon_case(name)
    wide = torch.zeros(T, B + 3, 64, device=dev)                     # a strided view, neither packed nor at the start of its buffer
    wide[:, 1:B + 2, 3:3 + C] = torch.cat([x, x[:, :1]], 1).to(dev)  # (line B: line 0 again, sent to row -1)
    view = wide[:, 1:B + 2, 3:3 + C]
    assert view.stride() == ((B + 3) * 64, 64, 1) and view.storage_offset() == 67
    pool = torch.full((B + 1, len(lex) + 6), 12345.0, dtype=torch.float64, device=dev)
    scores = pool[:, 2:2 + len(lex)]                                 # rows further apart than K
    with pytest.raises(ValueError):
        read.ctc_lexicon_score(view, lex, pool)
    read.ctc_lexicon_score(view, lex, scores)
    n_rows = B + 3
    order = [n_rows - 2 - b for b in range(B)] + [-1]                # reverse order into a larger record
    width = read.lexicon_record_words(nbest)
    rec = torch.full((n_rows, width + 5), FILL, dtype=torch.int32, device=dev)
    read.ctc_lexicon_select(scores, torch.tensor(order, dtype=torch.int32).to(dev), rec, nbest)
    host, pool_host = rec.cpu(), pool.cpu()
    assert bool((pool_host[:, :2] == 12345.0).all()) and bool((pool_host[:, 2 + len(lex):] == 12345.0).all())
    for r in range(n_rows):
        if r not in order:
            assert bool((host[r] == FILL).all()), r                  # untouched rows keep their fill
    assert bool((host[:, width:] == FILL).all())
    plain, plain_dec, _ = _run(dev, x, lex, nbest)
    assert torch.equal(pool_host[:B, 2:2 + len(lex)].contiguous().view(torch.int64), plain.view(torch.int64))
    assert torch.equal(pool_host[B, 2:2 + len(lex)].contiguous().view(torch.int64), plain[0].view(torch.int64))
    got = read.parse_lexicon_records(host[[order[b] for b in range(B)]][:, :width].contiguous(), nbest)
    assert got == plain_dec and [[k for k, _ in g.entries] for g in got] == [[k for k, _ in d.entries] for d in dec]
    rec.fill_(FILL)
    read.ctc_lexicon_select(scores, torch.tensor([-1, n_rows, -5, 2 ** 30], dtype=torch.int32).to(dev), rec, nbest)
    assert bool((rec == FILL).all())                                 # no index inside 0 .. n_rows - 1: nothing is written
    with pytest.raises(ValueError):
        read.ctc_lexicon_select(scores, torch.arange(B + 1, dtype=torch.int32).to(dev), rec, 17)
    with pytest.raises(ValueError):
        read.ctc_lexicon_select(scores, torch.arange(B + 1, dtype=torch.int32).to(dev), rec[:, :width - 1], nbest)
    with pytest.raises(ValueError):
        read.ctc_lexicon_score(view, lex, scores.to(torch.float32))
    torch.cuda.synchronize()
    assert bool((rec == FILL).all())


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
SOURCES = ((16, 64), (16, 72), (16, 76))                             # rw 100, 120, 120: a bucket of one line and a bucket of two
WORDS = random_words(ABC, 20, (2, 3, 4, 5, 6, 8), 51)


@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


def _census(read, ops):
    """count the decode launches of the reader and every library call that goes through ops.call, as tools/bench_read.py does"""
    names = ("ctc_greedy_read", "ctc_beam_read", "ctc_lexicon_score", "ctc_lexicon_select", "line_luma")
    census, calls, real, real_call = {k: 0 for k in names}, [], {k: getattr(read, k) for k in names}, ops.call

    def counted(name):
        def run(*a):
            census[name] += 1
            return real[name](*a)
        return run

    def counted_call(name, *a):
        calls.append(name)
        return real_call(name, *a)

    def start():
        for k in names:
            setattr(read, k, counted(k))
        ops.call = counted_call

    def stop():
        for k in names:
            setattr(read, k, real[k])
        ops.call = real_call
    return census, calls, start, stop


def test_line_reader_with_a_lexicon(dev, crnn):
    """every LexiconReading equals the specification run on the reader's own logits (kept, copied to the host): words and order exactly,
    logp within the bar of those logits, the posterior within what that leaves of exp(logp - logz); the kept scores are what was read"""
    from tatt_amd import ops, read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    images = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result()
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    lex = read.Lexicon(WORDS)
    reader = read.LineReader(crnn, batch_size=8, keep_logits=True, decode="lexicon", lexicon=lex, nbest=4, keep_scores=True)
    assert reader.lexicon is lex and read.LineReader(crnn, decode="lexicon", lexicon=WORDS).lexicon.words == WORDS
    census, calls, start, stop = _census(read, ops)
    torch.cuda.synchronize()
    start()
    try:
        torch.cuda.set_sync_debug_mode("error")                      # nothing waits for the device before result()
        try:
            pending = reader.read(buf, rows, 2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        stop()
    assert census == {"ctc_greedy_read": 0, "ctc_beam_read": 0, "ctc_lexicon_score": 2, "ctc_lexicon_select": 2, "line_luma": 1}
    readings = pending.result()
    assert [idx for idx, _ in pending.logits] == [idx for idx, _ in pending.scores] == [[0], [1, 2]]
    assert [(r.rw, r.squeezed) for r in readings] == [(100, False), (120, False), (120, False)]
    assert pending.texts() == [r.text for r in readings] and all(isinstance(r, read.LexiconReading) for r in readings)
    for (idx, lg), (_, sc) in zip(pending.logits, pending.scores):
        host = lg.cpu()
        assert tuple(sc.shape) == (len(idx), len(lex)) and sc.dtype == torch.float64
        want, bar, dist = spec_bar(host, lex)
        dec = read.ctc_lexicon_read_host(host, lex, 4, details=True, scores=want)
        worst = _compare_scores(sc.cpu(), want, bar, "reader")
        for j, i in enumerate(idx):
            w, r = dec[j], readings[i]
            print("line %d: bar %.3g (float64 - longdouble %.3g), device - specification %.3g, margin %.3g" % (i, bar, dist, worst,
                                                                                                             w.margin))
            assert w.flag == 0 and w.margin > 100 * bar
            assert [t for t, _, _ in r.alternatives] == [lex.words[k] for k, _ in w.entries] and len(r.alternatives) == 4
            assert [v for _, v, _ in r.alternatives] == [float(sc[j, k]) for k, _ in w.entries]
            assert (r.text, r.logp, r.posterior) == r.alternatives[0] and r.text in WORDS
            for (_, logp, post), (k, v) in zip(r.alternatives, w.entries):
                # exp has slope <= 1 below 0, so the posterior is as good as logp - logz (two bars and the K-term sum), one rounding of
                # that difference on either side and one of exp
                assert abs(logp - v) <= bar
                assert abs(post - math.exp(v - w.logz)) <= 2 * bar + len(lex) * 2.0 ** -52 + 2.0 ** -52 * (1 + abs(v - w.logz))
                assert 0.0 < post <= 1.0
    assert not reader.read(buf, [], 2).result() and read.LineReader(crnn, decode="lexicon", lexicon=lex).read(buf, rows, 2).scores is None


def test_super_resolver_reads_against_a_lexicon(dev, crnn):
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    from tests.test_quads_device_gpu import QUADS
    from tests.test_scene_device_gpu import BOXES
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    up = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_decode="lexicon", read_lexicon=WORDS, read_nbest=3)
    assert (up.reader.decode, up.reader.nbest, up.reader.lexicon.words) == ("lexicon", 3, WORDS)
    p = up(imgs)
    images, texts = p.result()
    _same(images, SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result())
    rs = p.readings()
    assert texts == [r.text for r in rs] and all(t in WORDS for t in texts) and len(texts) == 3
    assert all(isinstance(r, read.LexiconReading) and len(r.alternatives) == 3 and r.logp <= 0.0 and 0.0 < r.posterior <= 1.0 for r in rs)
    assert [(r.rw, r.squeezed) for r in rs] == [(100, False), (120, False), (120, False)]
    lex = read.Lexicon(WORDS, min_segment=64)
    scene_up = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn, read_decode="lexicon", read_lexicon=lex)
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32)
    for scene, regions, run, run_plain in ((_img(60, 48, 160, 1), BOXES, scene_up.scene, plain.scene),
                                           (_img(61, 97, 211, 1), QUADS, scene_up.scene_quads, plain.scene_quads)):
        q = run(scene, regions, 2)
        _same([q.result()], [run_plain(scene, regions, 2).result()])
        rs = q.readings()
        assert len(rs) == len(regions) and q.texts() == [r.text for r in rs] and all(r.text in WORDS for r in rs)
        assert all(isinstance(r, read.LexiconReading) and 1 <= len(r.alternatives) <= 4 and not math.isnan(r.logp) for r in rs)
    with pytest.raises(ValueError, match="lexicon="):
        SuperResolver(gen, reader=crnn, read_decode="lexicon")
    with pytest.raises(ValueError, match="nbest <= 16"):
        SuperResolver(gen, reader=crnn, read_decode="lexicon", read_lexicon=WORDS, read_nbest=17)


def test_greedy_and_beam_enqueue_what_they_enqueued(dev, crnn):
    """without the new keywords a call makes no lexicon launch, the decode launches it made before (one per bucket chunk), and the
    same library calls through ops.call in the same order under every decoding: the forward does not know how its logits are decoded"""
    from tatt_amd import ops, read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    images = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)([_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]).result()
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    seen = {}
    for decode, kw in (("greedy", {}), ("beam", {"beam": 8, "nbest": 4}), ("lexicon", {"lexicon": WORDS})):
        reader = read.LineReader(crnn, batch_size=8, decode=decode, **kw)
        reader.read(buf, rows, 2).result()                           # (folds and packs are made)
        census, calls, start, stop = _census(read, ops)
        start()
        try:
            pending = reader.read(buf, rows, 2)
        finally:
            stop()
        pending.result()
        assert pending.scores is None
        seen[decode] = (census, calls)
    assert seen["greedy"][0] == {"ctc_greedy_read": 2, "ctc_beam_read": 0, "ctc_lexicon_score": 0, "ctc_lexicon_select": 0, "line_luma": 1}
    assert seen["beam"][0] == {"ctc_greedy_read": 0, "ctc_beam_read": 2, "ctc_lexicon_score": 0, "ctc_lexicon_select": 0, "line_luma": 1}
    assert seen["greedy"][1].count("tatt_ctc_greedy_read") == 2 and not any("lexicon" in c for c in seen["greedy"][1] + seen["beam"][1])
    forward = [c for c in seen["greedy"][1] if c != "tatt_ctc_greedy_read"]
    assert len(forward) >= 2 and seen["beam"][1] == forward and seen["lexicon"][1] == forward
