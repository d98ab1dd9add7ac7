"""Reading lines of several words against a lexicon on the host (tatt_amd/read.py: ctc_words_host, ctc_words_read_host, WordSpan,
parse_words_records), the specification of csrc/ctcwords.hip, and what of the entry needs no GPU.  Yardstick: brute force over all C^T
alignments, the path sum taken step by step from t = 0, so that the best score is compared with ==.  CASES and the planted lines are the
shapes tests/test_words_device_gpu.py runs on the device."""
import itertools
import math
import random
import struct

import pytest
import torch

from tests.test_beam import beam_logits
from tests.test_lexicon import ABC, ABC64

ABC27 = "-abcdefghijklmnopqrstuvwxyz"
NEG = -math.inf
PLANT_WORDS = ["stop", "ahead", "only", "a", "head", "top", "on", "exit", "left"]      # sub-words beside the words that hold them
PLANT_T, PLANT_SEEDS = 64, range(50)
_cache = {}


def words_of(alphabet, lengths, seed):
    """one distinct word over alphabet[1:] per entry of `lengths`; the first word of every length >= 2 starts with a doubled letter"""
    rng, out, seen, doubled = random.Random(seed), [], set(), set()
    for L in lengths:
        for attempt in range(1000):
            w = [rng.choice(alphabet[1:]) for _ in range(L)]
            if L >= 2 and L not in doubled:
                w[1] = w[0]
            w = "".join(w)
            if w not in seen:
                break
        else:
            raise AssertionError("not enough distinct words of length %d" % L)
        doubled.add(L)
        seen.add(w)
        out.append(w)
    return out


def limit_lengths(lanes):
    """the lengths of a list that fills `lanes` packed lanes exactly: half of them in segments of 16, a quarter each in 32 and 64"""
    rng = random.Random(7)
    return ([rng.choice((3, 4, 5, 6, 7)) for _ in range(lanes // 2 // 16)] + [rng.choice((8, 11, 15)) for _ in range(lanes // 4 // 32)] +
            [rng.choice((16, 24, 31)) for _ in range(lanes // 4 // 64)])


# name -> (T, n, C, alphabet, lengths of the words or the words, word_penalty, seed of the logits)
def cases():
    from tatt_amd import read
    lanes = read.words_limits()["lanes"]
    return {"one-step": (1, 1, 2, "-a", ["a"], 0.0, 61),
            "all-6": (3, 2, 3, "-ab", ["a", "b", "aa", "ab", "ba", "bb"], 0.0, 62),
            "reader-T": (26, 3, 37, ABC, tuple(1 + i % 12 for i in range(50)), 0.0, 63),
            "every-class": (64, 5, 37, ABC, tuple((1, 2, 5, 7, 8, 15, 16, 31)[i % 8] for i in range(96)), 0.0, 64),
            "lane-limit": (256, 2, 37, ABC, tuple(limit_lengths(lanes)), 0.0, 65),
            "both-limits": (256, 1, 64, ABC64, (1, 3, 7, 12, 20, 31), 0.0, 66),
            "penalty-minus": (26, 3, 37, ABC, tuple(1 + i % 6 for i in range(40)), -2.5, 67),
            "penalty-plus": (26, 3, 37, ABC, tuple(1 + i % 6 for i in range(40)), 0.5, 68)}


def case_inputs(name):
    """-> (logits, lexicon, word_penalty); computed once and shared, never changed"""
    if name not in _cache:
        from tatt_amd import read
        T, n, C, alphabet, words, wp, seed = cases()[name]
        if isinstance(words, tuple):
            words = words_of(alphabet, words, seed + 100)
        _cache[name] = (beam_logits(T, n, C, 3.0, seed), read.Lexicon(words, alphabet=alphabet), wp)
    return _cache[name]


def log_softmax_rows(x, b, real=None):
    """the specification's log-soft-max of line b of (T, B, C) logits, as lists"""
    from tatt_amd import read
    r, exp, log, _ = read._beam_real(real)
    return [read._log_softmax_row(row, r, exp, log) for row in x[:, b].to(torch.float32).tolist()]


def collapse(path):
    """-> (string, runs): the collapsed classes and (first step, last step) of every character's run"""
    string, runs, last = [], [], 0
    for t, c in enumerate(path):
        if c != 0 and c != last:
            string.append(c)
            runs.append([t, t])
        elif c != 0:
            runs[-1][1] = t
        last = c
    return tuple(string), runs


def in_closure(string, words):
    ok = [True] + [False] * len(string)
    for i in range(len(string)):
        if ok[i]:
            for w in words:
                if w and string[i:i + len(w)] == tuple(w):
                    ok[i + len(w)] = True
    return ok[len(string)]


def brute_force_words(lp, lexicon):
    """-> (the largest path sum over the alignments whose collapsed string is a concatenation of list words, those alignments)"""
    T, C = len(lp), len(lp[0])
    best, paths = NEG, []
    for path in itertools.product(range(C), repeat=T):
        string, _ = collapse(path)
        if not in_closure(string, lexicon.classes):
            continue
        v = lp[0][path[0]]
        for t in range(1, T):
            v = v + lp[t][path[t]]
        if v > best:
            best, paths = v, [path]
        elif v == best:
            paths.append(path)
    return best, paths


def spans_fit(dec, lexicon, path):
    """the reported words spell the path's string and every word's first run starts at `first`, its last run ends at `last`"""
    string, runs = collapse(path)
    if tuple(c for k, _, _ in dec.words for c in lexicon.classes[k]) != string:
        return False
    o = 0
    for k, first, last in dec.words:
        L = len(lexicon.classes[k])
        if runs[o][0] != first or runs[o + L - 1][1] != last:
            return False
        o += L
    return True


def test_the_best_score_equals_brute_force_bit_for_bit():
    from tatt_amd import read
    rng, cases_run, with_words, several = random.Random(5), 0, 0, 0
    for case in range(240):
        T, nw = rng.randint(1, 6), rng.randint(1, 4)
        words = set()
        while len(words) < nw:
            words.add("".join(rng.choice("ab") for _ in range(rng.randint(1, 3))))
        lex = read.Lexicon(sorted(words, key=lambda w: rng.random()), alphabet="-ab")
        x = beam_logits(T, 1, 3, 3.0, 1000 + case)
        if case % 7 == 0:
            x[rng.randrange(T), 0, rng.randrange(3)] = NEG           # -inf logits are legal
        lp = log_softmax_rows(x, 0)
        dec = read.ctc_words_host(lp, lex)
        best, paths = brute_force_words(lp, lex)
        assert dec.logp == best and dec.flag == 0, (case, dec, best)
        assert in_closure(tuple(c for k, _, _ in dec.words for c in lex.classes[k]), lex.classes)
        assert any(spans_fit(dec, lex, p) for p in paths), (case, dec, paths)
        assert read.ctc_words_read_host(x, lex)[0] == dec
        cases_run, with_words, several = cases_run + 1, with_words + bool(dec.words), several + (len(dec.words) >= 2)
    assert cases_run == 240 and with_words > 120 and several > 40    # no case is left out, and words are read


def planted_path(string, T=7):
    """log-probabilities (T x 27) that put 0.74 on the given class of every step and 0.01 on each other class"""
    lp = [[math.log(0.01)] * 27 for _ in range(T)]
    for t, ch in enumerate(string):
        lp[t][ABC27.index(ch)] = math.log(0.74)
    return lp


def test_the_order_of_the_list_decides_ties_and_the_penalty_prefers_longer_words():
    from tatt_amd import read
    lp = planted_path("to-day-")
    texts = lambda lex, d: [(lex.words[k], a, b) for k, a, b in d.words]
    first = read.Lexicon(["to", "day", "today"], alphabet=ABC27)
    other = read.Lexicon(["today", "to", "day"], alphabet=ABC27)
    a, b = read.ctc_words_host(lp, first), read.ctc_words_host(lp, other)
    assert texts(first, a) == [("to", 0, 1), ("day", 3, 5)] and texts(other, b) == [("today", 0, 5)]
    assert a.logp == b.logp                                          # one alignment, two segmentations: an exact tie
    for lex in (first, other):
        d = read.ctc_words_host(lp, lex, word_penalty=-2.5)
        assert texts(lex, d) == [("today", 0, 5)] and d.logp == a.logp + -2.5
    lp = planted_path("today--")                                     # no blank inside: the same three readings
    assert texts(first, read.ctc_words_host(lp, first)) == [("to", 0, 1), ("day", 2, 4)]
    assert texts(other, read.ctc_words_host(lp, other)) == [("today", 0, 4)]


def test_words_follow_each_other_without_a_blank_only_across_different_classes():
    from tatt_amd import read
    lex = read.Lexicon(["ab", "ba"], alphabet="-ab")
    ok = [[NEG, 0.0, NEG], [NEG, NEG, 0.0], [0.0, NEG, NEG], [NEG, NEG, 0.0], [NEG, 0.0, NEG]]      # a b - b a
    d = read.ctc_words_host(ok, lex)
    assert d.words == [(0, 0, 1), (1, 3, 4)] and d.logp == 0.0
    forced = [[NEG, 0.0, NEG], [NEG, NEG, 0.0], [NEG, NEG, 0.0], [NEG, 0.0, NEG]]                    # a b b a: one word "aba", not in the list
    assert read.ctc_words_host(forced, lex) == read.WordsDecoded([], NEG, 0)
    # noisy lines of 4 and 5 steps that favour a b b a and a b (b or blank) b a: "ab" + "ba" needs 5 steps and the blank; wherever one
    # word's last class is the next word's first, a blank lies between
    seen = 0
    for T, favoured, seed in ((4, (1, 2, 2, 1), 77), (5, (1, 2, 2, 2, 1), 78), (5, (1, 2, 2, 2, 1), 79), (4, (1, 2, 1, 2), 80)):
        x = beam_logits(T, 1, 3, 0.3, seed)
        for t, c in enumerate(favoured):
            x[t, 0, c] += 5.0
        if T == 5:
            x[2, 0, 0] += 4.0
        lp = log_softmax_rows(x, 0)
        d = read.ctc_words_host(lp, lex)
        best, paths = brute_force_words(lp, lex)
        assert d.logp == best and any(spans_fit(d, lex, p) for p in paths)
        if T == 5:
            assert d.words == [(0, 0, 1), (1, 3, 4)]
        for (k1, _, l1), (k2, f2, _) in zip(d.words, d.words[1:]):
            seen += 1
            assert f2 >= l1 + (2 if lex.classes[k1][-1] == lex.classes[k2][0] else 1), (T, d)
    # the doubled letter of "abba" needs its blank too: 4 steps do not hold the word, the empty reading remains
    assert read.ctc_words_host(log_softmax_rows(beam_logits(4, 1, 3, 1.0, 77), 0), read.Lexicon(["abba"], alphabet="-ab")).words == []
    assert seen >= 3


def test_the_empty_word_is_ignored_and_a_line_nothing_can_spell():
    from tatt_amd import read
    x = beam_logits(6, 2, 4, 3.0, 81)
    with_empty, without = read.Lexicon(["", "ab", "c"], alphabet="-abc"), read.Lexicon(["ab", "c"], alphabet="-abc")
    a, b = read.ctc_words_read_host(x, with_empty), read.ctc_words_read_host(x, without)
    assert [(d.logp, [(k - 1, f, l) for k, f, l in d.words]) for d in a] == [(d.logp, d.words) for d in b]
    only_empty = read.ctc_words_read_host(x, read.Lexicon([""], alphabet="-abc"))
    for b_, d in enumerate(only_empty):                              # the empty reading: all blanks
        lp = log_softmax_rows(x, b_)
        v = lp[0][0]
        for t in range(1, 6):
            v = v + lp[t][0]
        assert d == read.WordsDecoded([], v, 0)
    x[:, 1, 0] = NEG                                                 # no blank and no "a": nothing of ["ab"] can be spelled
    x[:, 1, 1] = NEG
    got = read.ctc_words_read_host(x, read.Lexicon(["ab"], alphabet="-abc"))
    assert got[1] == read.WordsDecoded([], NEG, 0) and got[0].flag == 0 and got[0].logp > NEG


def degenerate_word_lines():
    """six lines of 6 steps and 4 classes: clean, a NaN, a +inf, a step without a finite logit, a -inf blank, and one nothing of the
    list can spell -> (logits, lexicon, flags)"""
    from tatt_amd import read
    x = beam_logits(6, 6, 4, 3.0, 40)
    x[2, 1, 3] = float("nan")
    x[5, 2, 0] = math.inf
    x[3, 3] = NEG
    x[:, 4, 0] = NEG
    x[:, 5, 0] = NEG                                                 # no blank, no "a" and no "b": "c" alone cannot be followed by "c"
    x[:, 5, 1] = NEG
    x[:, 5, 2] = NEG
    return x, read.Lexicon(["a", "ab", "abc", "ca", "cab", "b"], alphabet="-abc"), [0, 1, 1, 1, 0, 0]


def test_flagged_lines_and_the_penalty_argument():
    from tatt_amd import read
    x, lex, flags = degenerate_word_lines()
    got = read.ctc_words_read_host(x, lex)
    assert [g.flag for g in got] == flags
    for g in got[1:4]:
        assert g.words == [] and math.isnan(g.logp)
    assert got[4].words and got[4].logp > NEG                        # without a blank words still follow each other
    assert got[5] == read.WordsDecoded([], NEG, 0)
    for bad in (math.nan, math.inf, -math.inf, "1", None, True):
        with pytest.raises(ValueError, match="word_penalty"):
            read.ctc_words_host([[0.0, NEG]], read.Lexicon(["a"], alphabet="-a"), bad)
        with pytest.raises(ValueError, match="word_penalty"):
            read.ctc_words_read_host(x, lex, bad)
    with pytest.raises(ValueError, match="38 classes"):
        read.ctc_words_read_host(torch.zeros(2, 1, 37), read.Lexicon(["a"], alphabet=ABC + "!"))
    r = read._words_reading(got[1], lex, 120, True, 240)
    assert r == read.WordsReading("", r.logp, [], 120, True) and math.isnan(r.logp)


def planted_line(seed):
    """-> (the (64, 27) logits, the planted string, per character (first step, last step) of its run): four words of PLANT_WORDS, every
    character a run of 1 to 2 steps behind 0 to 2 blanks (at least one between equal letters); randn, + 8 at the planted class"""
    rng = random.Random(9000 + seed)
    for attempt in range(100):
        string = "".join(rng.choice(PLANT_WORDS) for _ in range(4))
        path, runs = [], []
        for i, ch in enumerate(string):
            blanks = rng.randint(0, 2)
            if i and string[i - 1] == ch:
                blanks = max(blanks, 1)
            path += [0] * blanks
            n = rng.randint(1, 2)
            runs.append((len(path), len(path) + n - 1))
            path += [ABC27.index(ch)] * n
        if len(path) <= PLANT_T:
            break
    else:
        raise AssertionError("no layout of %r fits %d steps" % (string, PLANT_T))
    path += [0] * (PLANT_T - len(path))
    x = torch.randn(PLANT_T, 27, generator=torch.Generator().manual_seed(9000 + seed), dtype=torch.float64)
    for t, c in enumerate(path):
        x[t, c] += 8.0
    return x.to(torch.float32), string, runs


def planted_lines(seeds):
    """-> ((64, n, 27) logits, [(string, runs)], the lexicon)"""
    from tatt_amd import read
    made = [planted_line(s) for s in seeds]
    return torch.stack([m[0] for m in made], 1), [(m[1], m[2]) for m in made], read.Lexicon(PLANT_WORDS, alphabet=ABC27)


def check_planted(dec, lexicon, string, runs):
    """the space-stripped reading is the planted string and every word's span lies inside the planted runs of its characters"""
    assert "".join(lexicon.words[k] for k, _, _ in dec.words) == string and dec.flag == 0, (dec, string)
    o = 0
    for k, first, last in dec.words:
        L = len(lexicon.words[k])
        assert runs[o][0] <= first <= last <= runs[o + L - 1][1], (dec, string, runs)
        o += L


def test_planted_lines_are_recovered_on_every_seed():
    from tatt_amd import read
    x, planted, lex = planted_lines(PLANT_SEEDS)
    got = read.ctc_words_read_host(x, lex)
    assert len(got) == len(PLANT_SEEDS) == 50
    for d, (string, runs) in zip(got, planted):
        check_planted(d, lex, string, runs)
    assert len({s for s, _ in planted}) > 40


def test_limits_header_and_refusals():
    import ctypes
    from tatt_amd import io, read
    from tatt_amd._lib import LIB, parse_header
    from tatt_amd.build import EXTRA_FLAGS, SOURCES
    lim = read.words_limits()
    out = (ctypes.c_int * 5)()
    assert LIB.tatt_words_limits(out) == 0 and LIB.tatt_words_limits(None) == 1
    assert [int(v) for v in out] == [lim[k] for k in ("steps", "classes", "lanes", "threads", "slots")]
    assert lim["lanes"] == lim["threads"] * lim["slots"] and lim["lanes"] % 64 == 0
    assert (lim["steps"], lim["classes"]) == (read.read_limits()["steps"], read.read_limits()["classes"])
    assert "ctcwords.hip" in SOURCES and "-ffp-contract=off" in EXTRA_FLAGS["ctcwords.hip"]
    protos = parse_header()
    assert [n for _, n in protos["tatt_ctc_words_read"]] == ["logits", "st_t", "st_b", "st_c", "T", "B", "C", "codes", "n_codes", "words",
                                                             "K", "k16", "k32", "k64", "word_penalty", "index", "record", "n_rows", "cap",
                                                             "st_rec", "lp_out", "st_lp", "st"]
    assert dict((n, t) for t, n in protos["tatt_ctc_words_read"])["word_penalty"] is ctypes.c_double
    assert io.ctc_words_host is read.ctc_words_host and io.WordsReading is read.WordsReading and io.words_limits is read.words_limits
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(logits=p, T=26, B=1, C=37, codes=p, n_codes=3, words=p, K=2, k16=2, k32=0, k64=0, wp=0.0, index=p, record=p, n_rows=1,
              cap=26, st_rec=56, lp_out=p, st_lp=26 * 37)
    over = lim["lanes"] // 64 + 1                                    # one segment of 64 lanes more than the limit
    for kw in ({"logits": None}, {"codes": None}, {"words": None}, {"index": None}, {"record": None}, {"T": 0}, {"T": 257}, {"C": 0},
               {"C": 65}, {"B": 0}, {"B": 65536}, {"K": 0}, {"K": 65537}, {"n_codes": -1}, {"k16": 1}, {"k16": 3, "k32": -1},
               {"K": over, "k16": 0, "k64": over}, {"K": lim["lanes"] // 16 + 1, "k16": lim["lanes"] // 16 + 1},
               {"K": lim["lanes"] // 16, "k16": lim["lanes"] // 16 - 1, "k32": 1}, {"wp": math.nan}, {"wp": math.inf}, {"wp": -math.inf},
               {"n_rows": 0}, {"cap": 25}, {"st_rec": 55}, {"st_lp": 26 * 37 - 1}):
        a = dict(ok, **kw)
        assert LIB.tatt_ctc_words_read(a["logits"], 37, 37, 1, a["T"], a["B"], a["C"], a["codes"], a["n_codes"], a["words"], a["K"],
                                       a["k16"], a["k32"], a["k64"], a["wp"], a["index"], a["record"], a["n_rows"], a["cap"], a["st_rec"],
                                       a["lp_out"], a["st_lp"], None) == 1, kw


def test_line_reader_keywords():
    from tatt_amd import read
    module = torch.nn.Linear(1, 1)                                   # the keywords are checked before the module is looked at
    with pytest.raises(ValueError, match="lexicon="):
        read.LineReader(module, decode="words")
    with pytest.raises(ValueError, match="lexicon="):
        read.LineReader(module, decode="beam", lexicon=["a"])
    with pytest.raises(ValueError, match="twice"):
        read.LineReader(module, decode="words", lexicon=["a", "A"])
    for decode, kw in (("greedy", {}), ("beam", {}), ("lexicon", {"lexicon": ["a"]})):
        with pytest.raises(ValueError, match="word_penalty= goes with decode='words'"):
            read.LineReader(module, decode=decode, word_penalty=-1.0, **kw)
    for bad in (math.nan, math.inf, "0", None):
        with pytest.raises(ValueError, match="word_penalty"):
            read.LineReader(module, decode="words", lexicon=["a"], word_penalty=bad)
    for decode in ("viterbi", "dictionary", "word"):
        with pytest.raises(ValueError, match="decode"):
            read.LineReader(module, decode=decode, lexicon=["a"])
    lanes = read.words_limits()["lanes"]
    fits = read.Lexicon(["%d" % i for i in range(10 ** 6, 10 ** 6 + lanes // 16)])
    over = read.Lexicon(fits.words + ["x"])
    assert read.words_lanes(fits) == lanes and read.words_lanes(over) == lanes + 64
    assert read.words_lanes(read.Lexicon(["a", "b" * 8, "c" * 16])) == 64 + 64 + 64
    with pytest.raises(ValueError, match="%d lanes.*at most %d" % (lanes + 64, lanes)):
        read.LineReader(module, decode="words", lexicon=over)
    import tatt_amd
    with pytest.raises(ValueError, match="emits 37"):
        read.LineReader(tatt_amd.CRNN(32, 1, 37, 8), decode="words", lexicon=read.Lexicon(["a"], alphabet=ABC64))
    with pytest.raises((AttributeError, ValueError, RuntimeError, StopIteration, TypeError)) as e:
        read.LineReader(module, decode="words", lexicon=fits, word_penalty=-0.5)      # the keywords pass; a Linear is no CRNN
    assert "lanes" not in str(e.value) and "word_penalty" not in str(e.value)


def test_word_spans_in_pixels():
    from tatt_amd import read
    assert read.word_span_pixels(0, 0, 200, 100) == (0, 4)           # the left edge: (4 * 0 - 2) is clipped to 0
    assert read.word_span_pixels(0, 25, 200, 100) == (0, 200)        # T = 26 at rw 100: the last step's 4 * 25 + 2 is clipped to W
    assert read.word_span_pixels(3, 7, 200, 100) == (20, 60)
    assert read.word_span_pixels(3, 7, 333, 180) == ((10 * 333) // 180, -(-(30 * 333) // 180)) == (18, 56)
    assert read.word_span_pixels(255, 255, 2040, 1020) == (2036, 2040)
    lex = read.Lexicon(["stop", "ahead"])
    r = read._words_reading(read.WordsDecoded([(0, 1, 9), (1, 12, 24)], -3.25, 0), lex, 100, False, 128)
    assert r.text == "stop ahead" and r.logp == -3.25 and (r.rw, r.squeezed) == (100, False)
    assert r.words == [read.WordSpan("stop", 0, 1, 9, 2, 49), read.WordSpan("ahead", 1, 12, 24, 58, 126)]
    assert "convention" in read.word_span_pixels.__doc__.lower()


def test_record_round_trip():
    from tatt_amd import read
    assert [read.words_record_words(c) for c in (1, 26, 256)] == [6, 56, 516]
    f64 = lambda v: list(struct.unpack("<ii", struct.pack("<d", v)))
    a = -0.1234567890123456789                                       # (not representable in fp32: the float64 travels as it is)
    rows = [[2, 0] + f64(a) + [7, 1 | 9 << 16, 65535, 12 | 255 << 16] + [-77] * 4,
            [0, 1] + f64(math.nan) + [-77] * 8,
            [0, 0] + f64(NEG) + [-77] * 8,
            [4, 0] + f64(0.0) + [0, 0, 1, 1 | 1 << 16, 0, 2 | 2 << 16, 3, 3 | 3 << 16]]
    got = read.parse_words_records(torch.tensor(rows, dtype=torch.int32), 4)
    assert got[0] == read.WordsDecoded([(7, 1, 9), (65535, 12, 255)], a, 0)
    assert got[1].words == [] and got[1].flag == 1 and math.isnan(got[1].logp)
    assert got[2] == read.WordsDecoded([], NEG, 0)
    assert got[3] == read.WordsDecoded([(0, 0, 0), (1, 1, 1), (0, 2, 2), (3, 3, 3)], 0.0, 0)
    with pytest.raises(ValueError):
        read.parse_words_records(torch.tensor([[5, 0] + [0] * 10], dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        read.parse_words_records(torch.tensor([[1, 0] + [0] * 9], dtype=torch.int32), 4)             # a row too short for cap
    with pytest.raises(ValueError):
        read.parse_words_records(torch.tensor([[0, 2] + [0] * 10], dtype=torch.int32), 4)


def test_the_device_cases_are_what_they_claim():
    from tatt_amd import read
    lim = read.words_limits()
    for name, (T, n, C, alphabet, words, wp, seed) in cases().items():
        if name == "lane-limit":
            continue                                                 # (its lexicon is made once, below)
        x, lex, _ = case_inputs(name)
        assert tuple(x.shape) == (T, n, C) and lex.n_classes == C and read.words_lanes(lex) <= lim["lanes"]
    _, lex, _ = case_inputs("lane-limit")
    assert read.words_lanes(lex) == lim["lanes"] and all(c > 0 for c in lex.counts)
    assert all(c > 0 for c in case_inputs("every-class")[1].counts) and case_inputs("reader-T")[1].counts[2] == 0
    assert sum(any(a == b for a, b in zip(w, w[1:])) for w in case_inputs("every-class")[1].words) >= 7
    big = case_inputs("every-class")[1].words
    assert len({w[0] for w in big}) < len(big) / 2 and len({w[-1] for w in big}) < len(big) / 2      # shared first and last letters
    assert (cases()["both-limits"][0], cases()["both-limits"][2]) == (lim["steps"], lim["classes"])
