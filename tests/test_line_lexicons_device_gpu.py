"""Reading every line against a lexicon of its own on the GPU (csrc/ctclexp.hip; read.ctc_lexicon_score_pairs,
read.ctc_lexicon_select_rows, read.LineReader(decode="lexicons"), infer.SuperResolver(read_decode="lexicons")).  Two yardsticks, in this
order of strength.  (1) The one-list path: for every line with a non-empty list the 64 bits of every score and the whole record row equal
what read.ctc_lexicon_score + read.ctc_lexicon_select write for that line's logits and Lexicon(its list) ALONE; the tolerance is zero
(the arithmetic of a word does not depend on where it sits: tests/test_lexicon_device_gpu.py).  (2) The host specification
read.ctc_line_lexicons_read_host: every finite score within the bar of tests/test_line_lexicons.py (from the specification alone: 4 x
|float64 - longdouble| + T x 2^-52 x max |score|), -inf and NaN equal as such, the entry ORDER on every line (behind margin > 100 x bar,
held on the CPU), logz within bar + K_b x 2^-52.  Shapes: tests/test_line_lexicons.py CASES."""
import math

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests.test_lexicon import ABC, random_words
from tests.test_line_lexicons import CASES, compare_with_spec, corrupt_tables, line_case
from tests.test_lines_device_gpu import LR, _generator, _img, _same
from tests.test_read_device_gpu import _upload

pytestmark = pytest.mark.gpu
FILL, SCORE_FILL, EXTRA = -77, 12345.0, 5


def _run(dev, x, lex, nbest, tables=None, index=None, n_rows=None):
    """the two launches on contiguous logits -> ((B, max count + EXTRA) float64 scores, the (n_rows, words + EXTRA) record), on the host;
    the scores are a view into a wider pool (rows further apart than the counts), everything pre-filled"""
    from tatt_amd import read
    B = x.shape[1]
    tiles, pairs, counts = tables if tables is not None else lex.pack(range(B))
    most = max(1, int(counts.max()))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pool = torch.full((B, most + EXTRA + 3), SCORE_FILL, dtype=torch.float64, device=dev)
    scores = pool[:, :most + EXTRA]
    index = list(range(B)) if index is None else index
    rec = torch.full((B if n_rows is None else n_rows, read.lexicon_record_words(nbest) + EXTRA), FILL, dtype=torch.int32, device=dev)
    counts_dev = up(counts)
    if len(tiles):
        read.ctc_lexicon_score_pairs(x.to(dev), up(lex.codes), lex.n_codes, up(lex.table), up(tiles), up(pairs), counts_dev, scores, most)
    read.ctc_lexicon_select_rows(scores, counts_dev, torch.tensor(index, dtype=torch.int32).to(dev), rec, nbest)
    pool = pool.cpu()
    assert bool((pool[:, most + EXTRA:] == SCORE_FILL).all())
    return pool[:, :most + EXTRA].contiguous(), rec.cpu()


def _alone(dev, row_logits, words, alphabet, nbest):
    """the ONE-LIST path on one line: logits (T, 1, C) on the device -> ((K,) float64 scores, the record row), on the host"""
    from tatt_amd import read
    lex = read.Lexicon(words, alphabet=alphabet)
    scores = torch.full((1, len(lex)), SCORE_FILL, dtype=torch.float64, device=dev)
    rec = torch.full((1, read.lexicon_record_words(nbest) + EXTRA), FILL, dtype=torch.int32, device=dev)
    read.ctc_lexicon_score(row_logits, lex, scores)
    read.ctc_lexicon_select(scores, torch.zeros(1, dtype=torch.int32, device=dev), rec, nbest)
    return scores.cpu()[0], rec.cpu()[0]


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("name", list(CASES))
def test_scores_and_records_equal_the_one_list_path_and_the_specification(dev, name):
    """Measured on an MI355X: see the README, section "Reading lines", paragraph "Per-line lexicons" (the bar and the distances)."""
    from tatt_amd import read
    x, lex, want, dec, bar, dist = line_case(name)
    T, n, C = x.shape
    nbest = CASES[name][5]
    scores, rec = _run(dev, x, lex, nbest)
    width = read.lexicon_record_words(nbest)
    xd = x.to(dev)
    for b, words in enumerate(lex.lists):
        if not words:                                                # entries 0, flag 0, logz = -inf, whatever the line is
            assert rec[b, :2].tolist() == [0, 0] and read.parse_lexicon_records(rec[b:b + 1, :width].contiguous(), nbest)[0].logz == -math.inf
            assert bool((rec[b, 4:] == FILL).all()) and bool((scores[b] == SCORE_FILL).all())
            continue
        one, one_rec = _alone(dev, xd[:, b:b + 1], words, lex.alphabet, nbest)
        assert torch.equal(_bits(scores[b, :len(words)]), _bits(one)), (name, b)                 # the 64 bits of every score
        assert torch.equal(rec[b], one_rec), (name, b, rec[b].tolist(), one_rec.tolist())          # entries, logz, flag, and the fill
    got = read.parse_lexicon_records(rec[:, :width].contiguous(), nbest)
    worst = compare_with_spec(name, scores, got, SCORE_FILL)
    for b, g in enumerate(got):
        assert bool((rec[b, 4 + 4 * len(g.entries):] == FILL).all()), (name, b)
    print("case %s (T %d, n %d, C %d, words %s, union %d, nbest %d): bar %.3g (float64 - longdouble of the specification %.3g), "
          "device - specification %.3g, smallest margin %.3g" % (name, T, n, C, [len(w) for w in lex.lists], len(lex.union), nbest, bar,
                                                                 dist, worst, min(d.margin for d in dec)))


def test_corrupt_tables_beside_clean_tiles_write_nothing(dev):
    """a tile whose line is out of range, a pair range past the end, a union position out of range, j >= count: scores and records are
    bit for bit what the clean tables give, the fill around them included.  (tools/line_lexicons_host_check.py ran these tables under the
    address sanitizer before the kernel's first launch on a GPU.)"""
    name = "reader-T"
    x, lex = line_case(name)[:2]
    nbest = CASES[name][5]
    clean, clean_rec = _run(dev, x, lex, nbest)
    tiles, pairs, counts = corrupt_tables(lex, 5)
    assert len(tiles) == len(lex.pack(range(5))[0]) + 10 and len(pairs) == int(counts.sum()) + 7
    scores, rec = _run(dev, x, lex, nbest, (tiles, pairs, counts))
    assert torch.equal(_bits(scores), _bits(clean)) and torch.equal(rec, clean_rec)
    short = counts.copy()
    short[0] = 7                                                     # a count below the pairs' j: those pairs are not written
    scores, rec = _run(dev, x, lex, nbest, (tiles, pairs, short))
    assert torch.equal(_bits(scores[0, :7]), _bits(clean[0, :7])) and bool((scores[0, 7:] == SCORE_FILL).all())
    for b in range(1, 5):                                            # (the buffer is as wide as the largest count left: 17)
        K = int(counts[b])
        assert torch.equal(_bits(scores[b, :K]), _bits(clean[b, :K])) and bool((scores[b, K:] == SCORE_FILL).all()), b
    assert torch.equal(rec[1:], clean_rec[1:])


def test_scattered_index(dev):
    name = "reader-T"
    x, lex = line_case(name)[:2]
    nbest = CASES[name][5]
    clean, clean_rec = _run(dev, x, lex, nbest)
    index = [6, -1, 0, 7, 3]
    scores, rec = _run(dev, x, lex, nbest, None, index, 7)
    assert torch.equal(_bits(scores), _bits(clean))
    for r in range(7):
        if r in index:
            assert torch.equal(rec[r], clean_rec[index.index(r)]), r
        else:
            assert bool((rec[r] == FILL).all()), r                   # rows without a valid index are untouched
    scores, rec = _run(dev, x, lex, nbest, None, [-1, 5, -7, 2 ** 30, 5], 5)
    assert bool((rec == FILL).all())


def test_the_wrappers_refuse_before_any_launch(dev):
    from tatt_amd import read
    x, lex = line_case("reader-T")[:2]
    tiles, pairs, counts = lex.pack(range(5))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    a = dict(logits=x.to(dev), codes=up(lex.codes), n_codes=lex.n_codes, table=up(lex.table), tiles=up(tiles), pairs=up(pairs),
             counts=up(counts), scores=torch.full((5, 50), SCORE_FILL, dtype=torch.float64, device=dev), max_count=50)
    rec = torch.full((5, read.lexicon_record_words(4)), FILL, dtype=torch.int32, device=dev)
    index = torch.arange(5, dtype=torch.int32, device=dev)
    for kw in (dict(scores=a["scores"][:, :49]), dict(scores=a["scores"].float()), dict(scores=a["scores"][:4]), dict(max_count=0),
               dict(tiles=a["tiles"][:0]), dict(tiles=a["tiles"].long()), dict(pairs=a["pairs"].view(-1)), dict(counts=a["counts"][:4]),
               dict(table=a["table"].cpu()), dict(n_codes=-1), dict(logits=torch.zeros(257, 5, 37, device=dev)),
               dict(logits=torch.zeros(26, 5, 65, device=dev))):
        with pytest.raises(ValueError):
            read.ctc_lexicon_score_pairs(**dict(a, **kw))
    for args in ((a["scores"], a["counts"], index, rec, 17), (a["scores"], a["counts"][:4], index, rec, 4),
                 (a["scores"], a["counts"], index, rec[:, :19], 4), (a["scores"].float(), a["counts"], index, rec, 4),
                 (a["scores"], a["counts"], index[:4], rec, 4)):
        with pytest.raises(ValueError):
            read.ctc_lexicon_select_rows(*args)
    torch.cuda.synchronize()
    assert bool((a["scores"] == SCORE_FILL).all()) and bool((rec == FILL).all())


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
SOURCES = ((16, 72), (16, 64), (16, 76))                             # rw 120, 100, 120: the buckets are [line 1], [lines 0, 2]
WORDS = random_words(ABC, 30, (2, 3, 4, 5, 6, 8), 151)
LISTS = [WORDS[:10], WORDS[10:20], WORDS[20:]]                       # disjoint: no word of a line's list is in another's


@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


def _census(read):
    names = ("ctc_greedy_read", "ctc_lexicon_score", "ctc_lexicon_select", "ctc_lexicon_score_pairs", "ctc_lexicon_select_rows", "line_luma")
    census, real = {k: 0 for k in names}, {k: getattr(read, k) for k in names}

    def counted(name):
        def run(*a):
            census[name] += 1
            return real[name](*a)
        return run

    def start():
        for k in names:
            setattr(read, k, counted(k))

    def stop():
        for k in names:
            setattr(read, k, real[k])
    return census, start, stop


def _alone_reading(dev, logits, j, words, nbest, rw):
    """the reading the one-list launches give line j of a chunk's kept logits against `words` alone"""
    from tatt_amd import read
    _, rec = _alone(dev, logits[:, j:j + 1], words, ABC, nbest)
    dec = read.parse_lexicon_records(rec[None, :read.lexicon_record_words(nbest)].contiguous(), nbest)[0]
    return read._lexicon_reading(dec, read.Lexicon(words), rw, False)


def _equal_readings(a, b):
    return a.text == b.text and a.rw == b.rw and a.squeezed == b.squeezed and len(a.alternatives) == len(b.alternatives) and all(
        p[0] == q[0] and np.float64(p[1]).tobytes() == np.float64(q[1]).tobytes() and np.float64(p[2]).tobytes() == np.float64(q[2]).tobytes()
        for p, q in zip([(a.text, a.logp, a.posterior)] + a.alternatives, [(b.text, b.logp, b.posterior)] + b.alternatives))


def test_line_reader_with_a_list_per_line(dev, crnn):
    """three lines whose bucket order [1, 0, 2] is not their input order: every reading equals, bit for bit, what the one-list launches
    give that line's kept logits against its own list alone; the same lists handed over in bucket order read differently"""
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    images = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result()
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    reader = read.LineReader(crnn, batch_size=8, keep_logits=True, decode="lexicons", nbest=4, keep_scores=True)
    reader.read(buf, rows, 2, lexicons=LISTS).result()               # (folds and packs are made)
    census, start, stop = _census(read)
    copies, real_copy = [], torch.Tensor.copy_

    def counted_copy(self, src, non_blocking=False):
        if self.is_cuda and not src.is_cuda:
            copies.append(tuple(src.shape))
        return real_copy(self, src, non_blocking=non_blocking)
    torch.cuda.synchronize()
    start()
    torch.Tensor.copy_ = counted_copy
    try:
        torch.cuda.set_sync_debug_mode("error")                      # nothing waits for the device before result()
        try:
            pending = reader.read(buf, rows, 2, lexicons=LISTS)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        torch.Tensor.copy_ = real_copy
        stop()
    assert census == {"ctc_greedy_read": 0, "ctc_lexicon_score": 0, "ctc_lexicon_select": 0, "ctc_lexicon_score_pairs": 2,
                      "ctc_lexicon_select_rows": 2, "line_luma": 1}
    assert len(copies) == 2                                          # the descriptor rows, and ONE blob of the union and all chunks' tables
    readings = pending.result()
    assert [idx for idx, _ in pending.logits] == [idx for idx, _, _ in pending.scores] == [[1], [0, 2]]
    assert [(r.rw, r.squeezed) for r in readings] == [(120, False), (100, False), (120, False)]
    assert all(isinstance(r, read.LexiconReading) and len(r.alternatives) == 4 and 0.0 < r.posterior <= 1.0 for r in readings)
    for (idx, lg), (_, sc, cnt) in zip(pending.logits, pending.scores):
        assert tuple(sc.shape) == (len(idx), 10) and sc.dtype == torch.float64 and cnt.tolist() == [10] * len(idx)
        for j, i in enumerate(idx):
            want = _alone_reading(dev, lg, j, LISTS[i], 4, readings[i].rw)
            assert _equal_readings(readings[i], want), (i, readings[i], want)
            assert readings[i].text in LISTS[i] and all(t in LISTS[i] for t, _, _ in readings[i].alternatives)
    order = [i for _, idx in pending._plan.buckets for i in idx]
    assert order == [1, 0, 2]
    swapped = reader.read(buf, rows, 2, lexicons=[LISTS[i] for i in order]).result()
    assert [r.text for r in swapped] != [r.text for r in readings] and swapped[0].text in LISTS[1] and swapped[1].text in LISTS[0]
    as_object = reader.read(buf, rows, 2, lexicons=read.LineLexicons(LISTS)).result()
    assert all(_equal_readings(a, b) for a, b in zip(as_object, readings))
    # an empty list reads "" beside lines that read as before
    some = reader.read(buf, rows, 2, lexicons=[LISTS[0], [], LISTS[2]]).result()
    assert some[1].text == "" and math.isnan(some[1].logp) and some[1].alternatives == [] and some[1].rw == 100
    assert _equal_readings(some[0], readings[0]) and _equal_readings(some[2], readings[2])
    none = reader.read(buf, rows, 2, lexicons=[[], [], []]).result()
    assert [r.text for r in none] == ["", "", ""]
    assert not reader.read(buf, [], 2, lexicons=[]).result()
    for bad, what in ((None, "needs lexicons="), (LISTS[:2], "2 lists of words for 3 lines"), ([["a", "A"], [], []], "twice")):
        with pytest.raises(ValueError, match=what):
            reader.read(buf, rows, 2, lexicons=bad)
    with pytest.raises(ValueError, match="decode='lexicons'"):
        read.LineReader(crnn, batch_size=8).read(buf, rows, 2, lexicons=LISTS)
    assert read.LineReader(crnn, decode="lexicons").read(buf, rows, 2, lexicons=LISTS).scores is None


def test_super_resolver_reads_every_item_against_its_own_list(dev, crnn):
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    from tests.test_polys_device_gpu import POLYS
    from tests.test_quads_device_gpu import QUADS
    from tests.test_scene_device_gpu import BOXES
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    up = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_decode="lexicons", read_nbest=3)
    assert (up.reader.decode, up.reader.nbest, up.reader.lexicon) == ("lexicons", 3, None)
    up.reader.keep_logits = True
    p = up(imgs, lexicons=LISTS)
    images, texts = p.result()
    _same(images, SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result())
    rs = p.readings()
    assert texts == [r.text for r in rs] and len(rs) == 3 and [r.rw for r in rs] == [120, 100, 120]
    for idx, lg in p._reading.logits:                                # one reading per image, in INPUT order
        for j, i in enumerate(idx):
            assert _equal_readings(rs[i], _alone_reading(dev, lg, j, LISTS[i], 3, rs[i].rw)), i
    for bad, what in ((None, "needs lexicons="), (LISTS[:2], "2 lists of words for 3 lines")):
        with pytest.raises(ValueError, match=what):
            up(imgs, lexicons=bad)
    empty = up([], lexicons=[])
    assert empty.result() == ([], []) and empty.readings() == []
    scene_up = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn, read_decode="lexicons", read_nbest=16)
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32)
    greedy = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn)
    for scene, regions, run, run_plain, run_greedy in (
            (_img(60, 48, 160, 1), BOXES, scene_up.scene, plain.scene, greedy.scene),
            (_img(61, 97, 211, 1), QUADS, scene_up.scene_quads, plain.scene_quads, greedy.scene_quads),
            (_img(62, 96, 200, 1), POLYS, scene_up.scene_polys, plain.scene_polys, greedy.scene_polys)):
        lists = [[] if k == 1 else WORDS[3 * k:3 * k + 7] for k in range(len(regions))]
        q = run(scene, regions, 2, lexicons=lists)
        picture = run_plain(scene, regions, 2).result()
        _same([q.result()], [picture])
        rs = q.readings()
        assert len(rs) == len(regions) and q.texts() == [r.text for r in rs]
        for k, r in enumerate(rs):
            assert isinstance(r, read.LexiconReading)
            if k == 1:
                assert r.text == "" and math.isnan(r.logp) and r.alternatives == []
            else:
                assert r.text in lists[k] and 1 <= len(r.alternatives) <= 7 and all(t in lists[k] for t, _, _ in r.alternatives)
                assert abs(sum(post for _, _, post in r.alternatives) - 1.0) <= 1e-9      # the posterior is taken among the line's OWN words
        with pytest.raises(ValueError, match="lists of words for"):
            run(scene, regions, 2, lexicons=lists[:-1])
        with pytest.raises(ValueError, match="needs lexicons="):
            run(scene, regions, 2)
        with pytest.raises(ValueError, match="decode='lexicons'"):
            run_greedy(scene, regions, 2, lexicons=lists)
        with pytest.raises(ValueError, match="reader="):
            run_plain(scene, regions, 2, lexicons=lists)
        # a reader without the new keyword: the picture and the readings it gave before, and no launch of the new kernels
        census, start, stop = _census(read)
        start()
        try:
            g = run_greedy(scene, regions, 2)
        finally:
            stop()
        _same([g.result()], [picture])
        assert census["ctc_lexicon_score_pairs"] == census["ctc_lexicon_select_rows"] == 0 and census["ctc_greedy_read"] >= 1
        assert len(g.readings()) == len(regions) and all(isinstance(r, read.Reading) for r in g.readings())
    with pytest.raises(ValueError, match="lexicon="):
        SuperResolver(gen, reader=crnn, read_decode="lexicons", read_lexicon=WORDS)
    with pytest.raises(ValueError, match="nbest <= 16"):
        SuperResolver(gen, reader=crnn, read_decode="lexicons", read_nbest=17)
