"""Reading lines against a lexicon on the host (tatt_amd/read.py: Lexicon, ctc_lexicon_scores_host, ctc_lexicon_read_host,
parse_lexicon_records), the specification of csrc/ctclex.hip, and what of the entries needs no GPU.  Yardstick: brute force over all C^T
alignments where that is possible.  CASES are the shapes tests/test_lexicon_device_gpu.py runs on the device; their seeds are held to the
margin condition here, so a bad seed fails without a GPU."""
import itertools
import math
import random
import struct

import numpy as np
import pytest
import torch

from tests.test_beam import beam_logits, brute_force

ABC = "-0123456789abcdefghijklmnopqrstuvwxyz"                        # the reader's alphabet, blank first
ABC64 = ABC + "".join(chr(0x3b1 + i) for i in range(27))             # 64 classes, the class limit (lower-case letters: lower() keeps them)
ALL15 = ["".join(p) for n in range(4) for p in itertools.product("ab", repeat=n)]    # every string of length <= 3 over two classes
EVERY_CLASS = (0, 1, 2, 5, 6, 7, 8, 10, 15, 16, 31)                  # lengths on both sides of the segment boundaries 7 | 8 and 15 | 16
# name -> (T, n, C, alphabet, words or (K, lengths), nbest, seed of the logits): the smallest shapes at which each path can go wrong
CASES = {"one-step": (1, 1, 2, "-a", ["", "a"], 2, 21),
         "all-15": (3, 2, 3, "-ab", ALL15, 15, 22),
         "reader-T": (26, 3, 37, ABC, (50, tuple(range(1, 13))), 4, 23),
         "every-class": (64, 5, 37, ABC, (96, EVERY_CLASS), 5, 24),
         "step-limit": (256, 2, 37, ABC, (33, (0, 1, 4, 9, 14, 19, 24, 28, 31)), 4, 25),
         "class-limit": (7, 1, 64, ABC64, (5, (1, 2, 3)), 1, 26),
         "lds-limit": (256, 1, 64, ABC64, (6, (0, 3, 7, 12, 20, 31)), 2, 27)}      # both limits at once: 68,608 bytes of staged logits
_cache = {}


def random_words(alphabet, K, lengths, seed):
    """K distinct words over alphabet[1:], their lengths taken in turn from `lengths`; the first word of every length >= 2 starts with
    a doubled letter (the recursion's no-skip rule)"""
    rng, out, seen, doubled, i = random.Random(seed), [], set(), set(), 0
    while len(out) < K:
        L = lengths[i % len(lengths)]
        i += 1
        assert i < 100 * K, "not enough distinct words of these lengths"
        w = [rng.choice(alphabet[1:]) for _ in range(L)]
        if L >= 2 and L not in doubled:
            w[1] = w[0]
            doubled.add(L)
        w = "".join(w)
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def case_lexicon(name, min_segment=16):
    from tatt_amd import read
    T, n, C, alphabet, words, nbest, seed = CASES[name]
    if isinstance(words, tuple):
        words = random_words(alphabet, words[0], words[1], seed + 100)
    return read.Lexicon(words, alphabet=alphabet, min_segment=min_segment)


def spec_bar(x, lexicon):
    """-> (float64 scores per line, bar, distance): the bar of the device tests, from the specification alone: 4 x the largest
    |float64 - longdouble| over the specification's finite scores + T x 2^-52 x the largest |finite score|"""
    from tatt_amd import read
    want = read.ctc_lexicon_scores_host(x, lexicon)
    wide = read.ctc_lexicon_scores_host(x, lexicon, real=np.longdouble)
    dist = top = 0.0
    for a, b in zip(want, wide):
        if a is None:
            assert b is None
            continue
        for v, w in zip(a, b):
            assert (v == -math.inf) == (w == -math.inf)
            if v != -math.inf:
                dist, top = max(dist, abs(float(np.longdouble(v) - w))), max(top, abs(v))
    return want, 4 * dist + x.shape[0] * 2.0 ** -52 * top, dist


def lexicon_case(name):
    """-> (logits, lexicon, float64 scores, decoded with details, bar, distance); computed once and shared, never changed"""
    if name not in _cache:
        from tatt_amd import read
        T, n, C, alphabet, words, nbest, seed = CASES[name]
        x, lex = beam_logits(T, n, C, 3.0, seed), case_lexicon(name)
        want, bar, dist = spec_bar(x, lex)
        _cache[name] = (x, lex, want, read.ctc_lexicon_read_host(x, lex, nbest, details=True, scores=want), bar, dist)
    return _cache[name]


def test_every_score_equals_brute_force():
    from tatt_amd import read
    x = beam_logits(3, 2, 3, 3.0, 22)
    lex = read.Lexicon(ALL15, alphabet="-ab")
    assert len(lex) == 15 and lex.classes[ALL15.index("aa")] == [1, 1]
    got = read.ctc_lexicon_read_host(x, lex, nbest=15, details=True)
    scores = read.ctc_lexicon_scores_host(x, lex)
    for b, g in enumerate(got):
        exact = brute_force(x[:, b])                                 # the 27 alignments, collapsed
        for k, w in enumerate(lex.classes):
            if tuple(w) in exact:
                assert abs(scores[b][k] - exact[tuple(w)]) <= 1e-14, (b, w)
            else:
                assert scores[b][k] == -math.inf, (b, w)
            assert scores[b][k] == read.ctc_string_logp_host(x[:, b], w)
        assert scores[b][ALL15.index("aa")] > -math.inf and scores[b][ALL15.index("aaa")] == -math.inf
        assert ALL15.index("aaa") not in [k for k, _ in g.entries] and all(v > -math.inf for _, v in g.entries)
        assert [k for k, _ in g.entries] == sorted((k for k in range(15) if scores[b][k] > -math.inf), key=lambda k: (-scores[b][k], k))
        assert set(exact) == {tuple(lex.classes[k]) for k, _ in g.entries}
        assert abs(g.logz - math.log(math.fsum(math.exp(v) for v in exact.values()))) <= 1e-14 and g.flag == 0
        assert g.margin == min(a[1] - c[1] for a, c in zip(g.entries, g.entries[1:]))
    short = read.ctc_lexicon_read_host(x, lex, nbest=2, details=True)
    assert [s.entries for s in short] == [g.entries[:2] for g in got] and [s.logz for s in short] == [g.logz for g in got]
    assert short[0].margin == min(got[0].entries[0][1] - got[0].entries[1][1], got[0].entries[1][1] - got[0].entries[2][1])
    assert read.ctc_lexicon_read_host(x, lex)[0].margin is None


def test_flagged_and_degenerate_lines_on_the_host():
    from tatt_amd import read
    x, lex, _ = degenerate_lines()
    got = read.ctc_lexicon_read_host(x, lex, nbest=4, details=True)
    assert [g.flag for g in got] == [0, 1, 1, 1, 0, 0]
    for g in got[1:4]:
        assert g.entries == [] and math.isnan(g.logz) and g.margin == math.inf
    assert len(got[4].entries) == 4 and not {"aa", "bcca"} & {lex.words[k] for k, _ in got[4].entries}    # no blank: no doubled letter
    assert got[5].entries == [] and got[5].logz == -math.inf and got[5].flag == 0 and got[5].margin == math.inf
    r = read._lexicon_reading(got[0], lex, 100, False)
    assert r.text == lex.words[got[0].entries[0][0]] and r.logp == got[0].entries[0][1] and len(r.alternatives) == 4
    assert abs(r.posterior - math.exp(r.logp - got[0].logz)) == 0.0 and 0.0 < r.posterior <= 1.0
    assert abs(sum(p for _, _, p in read._lexicon_reading(read.ctc_lexicon_read_host(x, lex, nbest=7)[0], lex, 100, False).alternatives)
               - 1.0) <= 1e-12
    for g in (got[1], got[5]):
        f = read._lexicon_reading(g, lex, 120, True)
        assert f.text == "" and math.isnan(f.logp) and f.alternatives == [] and f.rw == 120 and f.squeezed


def degenerate_lines():
    """six lines of 6 steps and 4 classes: clean, a NaN, a +inf, a step without a finite logit, no blank at all, and one on which no
    word of the lexicon has an alignment (class 1 is impossible and every word has an "a") -> (logits, lexicon, flags)"""
    from tatt_amd import read
    inf = float("inf")
    x = beam_logits(6, 6, 4, 3.0, 40)
    x[2, 1, 3] = float("nan")
    x[5, 2, 0] = inf
    x[3, 3] = -inf
    x[:, 4, 0] = -inf
    x[:, 5, 1] = -inf
    return x, read.Lexicon(["a", "ab", "abc", "aa", "cab", "aba", "bcca"], alphabet="-abc"), [0, 1, 1, 1, 0, 0]


def test_lexicon_mapping_and_refusals():
    from tatt_amd import io, read
    lex = read.Lexicon(["Hello", "", "a0", "ZZ"])
    assert lex.words == ["hello", "", "a0", "zz"] and len(lex) == 4 and lex.n_classes == 37
    assert lex.classes == [[18, 15, 22, 22, 25], [], [11, 1], [36, 36]] and lex.alphabet == "-" + io.ALPHABET == ABC
    assert read.Lexicon(["ba"], alphabet="-ab").classes == [[2, 1]]
    for words, what in ((["ok", "a-b"], "a-b"), (["ok", "café"], "caf"), (["x" * 32], "x" * 32), (["abc", "ABC"], "abc"), ([], "empty"),
                        (["a", "a"], "'a'")):
        with pytest.raises(ValueError, match=what):
            read.Lexicon(words)
    with pytest.raises(ValueError, match="65537"):
        read.Lexicon(["%d" % i for i in range(65537)])
    with pytest.raises(ValueError):
        read.Lexicon(["a"], min_segment=8)
    with pytest.raises(ValueError):
        read.Lexicon("abc")
    assert len(read.Lexicon(["x" * 31])) == 1
    assert io.Lexicon is read.Lexicon and io.LexiconReading is read.LexiconReading and io.ctc_lexicon_read_host is read.ctc_lexicon_read_host
    assert io.lexicon_limits is read.lexicon_limits


def test_lexicon_packing():
    from tatt_amd import read
    words = ["a" * L + "b" for L in (6, 7, 14, 15, 30)] + ["", "q"]      # lengths 7, 8, 15, 16, 31, 0, 1
    lex = read.Lexicon(words)
    assert lex.segments == [16, 32, 32, 64, 64, 16, 16] and lex.counts == (3, 2, 2)
    assert lex.order == [0, 5, 6, 1, 2, 3, 4] and sorted(lex.order) == list(range(7))      # every word exactly once
    assert lex.table.dtype == np.int32 and lex.table.shape == (7, 4) and lex.table[:, 2].tolist() == lex.order
    for p, k in enumerate(lex.order):
        L, off = int(lex.table[p, 0]), int(lex.table[p, 1])
        assert L == len(words[k]) and lex.codes[off:off + L].tolist() == lex.classes[k] and lex.table[p, 3] == 0
        assert 2 * L + 1 <= lex.segments[k]
    assert lex.n_codes == sum(len(w) for w in words) and len(lex.codes) == lex.n_codes + 1
    wide = read.Lexicon(words, min_segment=64)
    assert wide.segments == [64] * 7 and wide.counts == (0, 0, 7) and wide.order == list(range(7))
    mid = read.Lexicon(words, min_segment=32)
    assert mid.segments == [32, 32, 32, 64, 64, 32, 32] and mid.counts == (0, 5, 2)
    only = read.Lexicon([""])
    assert only.counts == (1, 0, 0) and only.n_codes == 0 and len(only.codes) == 1
    big = case_lexicon("every-class")
    assert sorted(big.order) == list(range(96)) and all(n > 0 for n in big.counts)
    assert {len(w) for w in big.words} == set(EVERY_CLASS)
    assert sum(any(a == b for a, b in zip(w, w[1:])) for w in big.words) >= 8          # doubled letters are among them


def test_limits_header_and_refusals():
    import ctypes
    from tatt_amd import read
    from tatt_amd._lib import LIB, parse_header
    from tatt_amd.build import SOURCES
    assert read.lexicon_limits() == {"steps": 256, "classes": 64, "length": 31, "words": 65536, "nbest": 16}
    assert (read.Lexicon.LENGTH, read.Lexicon.WORDS) == (31, 65536)
    assert (read.lexicon_limits()["steps"], read.lexicon_limits()["classes"]) == (read.read_limits()["steps"], read.read_limits()["classes"])
    assert "ctclex.hip" in SOURCES and "ctcbeam.hip" in SOURCES
    protos = parse_header()
    for name in ("tatt_ctc_lexicon_score", "tatt_ctc_lexicon_select", "tatt_lexicon_limits"):
        assert name in protos, name
    args = [n for _, n in protos["tatt_ctc_lexicon_score"]]
    for a in ("logits", "st_t", "st_b", "st_c", "T", "B", "C", "codes", "n_codes", "words", "K", "k16", "k32", "k64", "scores", "st_sc", "st"):
        assert a in args, a
    assert [n for _, n in protos["tatt_ctc_lexicon_select"]] == ["scores", "st_sc", "B", "K", "nbest", "index", "record", "n_rows",
                                                                 "st_rec", "st"]
    # null pointers and zero sizes: 1, before any launch (nothing here touches a device)
    assert LIB.tatt_lexicon_limits(None) == 1
    assert LIB.tatt_ctc_lexicon_score(None, 0, 0, 0, 26, 1, 37, None, 0, None, 1, 1, 0, 0, None, 1, None) == 1
    assert LIB.tatt_ctc_lexicon_select(None, 1, 1, 1, 1, None, None, 1, 8, None) == 1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    score = dict(T=26, B=1, C=37, n_codes=3, K=2, k16=2, k32=0, k64=0, st_sc=2)
    for kw in ({"T": 0}, {"T": 257}, {"C": 0}, {"C": 65}, {"B": 0}, {"B": 65536}, {"K": 0}, {"K": 65537}, {"n_codes": -1}, {"k16": 1},
               {"k16": 3, "k32": -1}, {"st_sc": 1}):
        a = dict(score, **kw)
        assert LIB.tatt_ctc_lexicon_score(p, 37, 37, 1, a["T"], a["B"], a["C"], p, a["n_codes"], p, a["K"], a["k16"], a["k32"], a["k64"],
                                          p, a["st_sc"], None) == 1, kw
    select = dict(st_sc=2, B=1, K=2, nbest=4, n_rows=1, st_rec=20)
    for kw in ({"B": 0}, {"K": 0}, {"K": 65537}, {"st_sc": 1}, {"nbest": 0}, {"nbest": 17}, {"n_rows": 0}, {"st_rec": 19}):
        a = dict(select, **kw)
        assert LIB.tatt_ctc_lexicon_select(p, a["st_sc"], a["B"], a["K"], a["nbest"], p, p, a["n_rows"], a["st_rec"], None) == 1, kw
    module = torch.nn.Linear(1, 1)                                   # the keywords are checked before the module is looked at
    with pytest.raises(ValueError, match="lexicon="):
        read.LineReader(module, decode="lexicon")
    with pytest.raises(ValueError, match="lexicon="):
        read.LineReader(module, decode="greedy", lexicon=["a"])
    with pytest.raises(ValueError, match="twice"):
        read.LineReader(module, decode="lexicon", lexicon=["a", "A"])
    for nbest in (0, 17, 4.0):
        with pytest.raises(ValueError, match="nbest <= 16"):
            read.LineReader(module, decode="lexicon", lexicon=["a"], nbest=nbest)
    with pytest.raises(ValueError, match="decode"):
        read.LineReader(module, decode="dictionary")


def test_more_classes_than_the_crnn_emits():
    import tatt_amd
    from tatt_amd import read
    crnn = tatt_amd.CRNN(32, 1, 37, 8)
    with pytest.raises(ValueError, match="emits 37"):
        read.LineReader(crnn, decode="lexicon", lexicon=read.Lexicon(["a"], alphabet=ABC64))
    with pytest.raises(ValueError, match="38 classes"):
        read.ctc_lexicon_scores_host(torch.zeros(2, 1, 37), read.Lexicon(["a"], alphabet=ABC + "!"))


def test_record_round_trip():
    from tatt_amd import read
    assert [read.lexicon_record_words(n) for n in (1, 4, 16)] == [8, 20, 68]
    f64 = lambda v: list(struct.unpack("<ii", struct.pack("<d", v)))
    a, z = -0.1234567890123456789, -0.0123456789012345678            # (not representable in fp32: the float64 travels as it is)
    rows = [[2, 0] + f64(z) + f64(a) + [7, 0] + f64(-7.5) + [0, 0] + [-77] * 4 + [-77] * 3,
            [0, 1] + f64(float("nan")) + [-77] * 15,
            [0, 0] + f64(-math.inf) + [-77] * 15,
            [3, 0] + f64(0.0) + f64(0.0) + [65535, 0] + f64(-1e-300) + [1, 0] + f64(-745.5) + [2, 0] + [-77] * 3]
    got = read.parse_lexicon_records(torch.tensor(rows, dtype=torch.int32), 3)
    assert got[0] == read.LexiconDecoded([(7, a), (0, -7.5)], z, 0)
    assert got[1].entries == [] and got[1].flag == 1 and math.isnan(got[1].logz)
    assert got[2] == read.LexiconDecoded([], -math.inf, 0)
    assert got[3] == read.LexiconDecoded([(65535, 0.0), (1, -1e-300), (2, -745.5)], 0.0, 0)
    lex = read.Lexicon(["w%d" % i for i in range(8)])
    r = read._lexicon_reading(got[0], lex, 120, False)
    assert r == read.LexiconReading("w7", a, math.exp(a - z), [("w7", a, math.exp(a - z)), ("w0", -7.5, math.exp(-7.5 - z))], 120, False)
    with pytest.raises(ValueError):
        read.parse_lexicon_records(torch.tensor([[4, 0] + [0] * 18], dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        read.parse_lexicon_records(torch.tensor([[1, 0] + [0] * 9], dtype=torch.int32), 3)           # a row too short for nbest


@pytest.mark.parametrize("name", list(CASES))
def test_the_seeds_of_the_device_cases_keep_the_margin(name):
    """the device test asserts the ORDER of a line's entries only behind margin > 100 x bar, and no line may be left out"""
    T, n, C, alphabet, words, nbest, seed = CASES[name]
    x, lex, want, dec, bar, dist = lexicon_case(name)
    assert tuple(x.shape) == (T, n, C) and lex.n_classes == C and len(dec) == n
    gap = min(d.margin for d in dec)
    print("%s: bar %.3g (float64 - longdouble %.3g), smallest neighbour gap %.3g, entries %s" % (name, bar, dist, gap,
                                                                                                [len(d.entries) for d in dec]))
    for b, d in enumerate(dec):
        assert d.flag == 0 and d.margin > 100 * bar, (name, b, d.margin, bar)
        assert len(d.entries) == min(nbest, sum(v > -math.inf for v in want[b]))
    if name == "every-class":                                        # words of every class are feasible at T = 64 (2 L - 1 <= 63 even doubled)
        assert all(v > -math.inf for row in want for v in row)
    if name == "all-15":
        assert any(v == -math.inf for v in want[0])


def test_the_ties_case_has_equal_scores():
    from tatt_amd import read
    lex = read.Lexicon(TIES, alphabet="-abcd")
    got = read.ctc_lexicon_read_host(torch.zeros(9, 2, 5), lex, nbest=6, details=True)
    for g in got:
        assert [k for k, _ in g.entries] == [0, 1, 2, 3, 4, 5] and len({v for _, v in g.entries}) == 1 and g.margin == 0.0


TIES = ["abcd", "dcba", "abab", "cdcd", "acbd", "bdac"]              # length 4, no adjacent repeats: the same recursion for each
