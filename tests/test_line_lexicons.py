"""Reading every line against a lexicon of its OWN on the host (tatt_amd/read.py: LineLexicons, ctc_line_lexicons_read_host), the
specification of csrc/ctclexp.hip, and what of the entries needs no GPU.  Yardsticks: the one-list specification
`ctc_lexicon_read_host` of every line alone (equal with ==) and brute force over all C^T alignments where that is possible.  CASES are
the shapes tests/test_line_lexicons_device_gpu.py and tools/line_lexicons_host_check.py run; their seeds are held to the margin
condition here, so a bad seed fails without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.test_beam import beam_logits, brute_force
from tests.test_lexicon import ABC, ABC64, ALL15, degenerate_lines, random_words, spec_bar

_SHORT = random_words(ABC, 60, tuple(range(1, 8)), 131)              # 2 L + 1 <= 16: segment class 16
_LONG = random_words(ABC, 21, tuple(range(8, 13)), 132)              # segment class 32
_SKEW = random_words(ABC, 300, (0, 1, 2, 5, 6, 7, 8, 10, 15, 16, 24, 31), 133)
_DEG = ["a", "ab", "abc", "aa", "cab", "aba", "bcca"]                # the words of tests.test_lexicon.degenerate_lines
# name -> (T, n, C, alphabet, one list per line, nbest, seed of the logits; None: the degenerate lines)
CASES = {
    "one-step": (1, 1, 2, "-a", [["", "a"]], 2, 21),                                       # no step loop; S = 1 and S = 3
    "all-15": (3, 2, 3, "-ab", [ALL15, ["ba", "", "a"]], 15, 22),                          # brute force; a word at another j on line 1
    # lists of 50, 1, 0, 17 and 16 words: classes 16 and 32, full tiles, a tile of one, an empty line, 16 | 17 words of one class
    "reader-T": (26, 5, 37, ABC, [_SHORT[:29] + _LONG, [_SHORT[3]], [], _SHORT[20:29] + _SHORT[40:48],
                                  _SHORT[7::-1] + _SHORT[48:56]], 4, 23),
    # one line of 300 words beside three of 3: class 64, many tiles for one line beside single tiles, doubled letters
    "skew": (64, 4, 37, ABC, [_SKEW[5:8], _SKEW, [_SKEW[299], _SKEW[0], _SKEW[150]], _SKEW[40:43]], 5, 24),
    "lds-limit": (256, 1, 64, ABC64, [random_words(ABC64, 6, (0, 3, 7, 12, 20, 31), 127)], 2, 27),       # 68,608 bytes of staged logits
    "degenerate": (6, 6, 4, "-abc", [_DEG, _DEG[::-1], _DEG[:3], ["cab", "a"], _DEG[2:], _DEG[1:5]], 4, None),
}
_cache = {}


def case_inputs(name):
    """-> (logits, LineLexicons, nbest)"""
    from tatt_amd import read
    T, n, C, alphabet, lists, nbest, seed = CASES[name]
    x = degenerate_lines()[0] if seed is None else beam_logits(T, n, C, 3.0, seed)
    return x, read.LineLexicons(lists, alphabet=alphabet), nbest


def line_case(name):
    """-> (logits, LineLexicons, float64 scores per line (None: flagged; [] for an empty list), decoded with details, bar, distance);
    the bar is tests.test_lexicon.spec_bar's formula over all lines of the case, from the specification alone: 4 x the largest
    |float64 - longdouble| over the finite scores + T x 2^-52 x the largest |finite score|.  Computed once and shared, never changed."""
    if name not in _cache:
        from tatt_amd import read
        x, lex, nbest = case_inputs(name)
        want, dist, top = [], 0.0, 0.0
        for b, words in enumerate(lex.lists):
            if not words:
                v = read.ctc_string_logp_host(x[:, b], [])           # (nan: a flagged line)
                want.append(None if v != v else [])
                continue
            row, _, d = spec_bar(x[:, b:b + 1], read.Lexicon(words, alphabet=lex.alphabet))
            want.append(row[0])
            dist = max(dist, d)
            top = max([top] + [abs(v) for v in row[0] or [] if v != -math.inf])
        bar = 4 * dist + x.shape[0] * 2.0 ** -52 * top
        _cache[name] = (x, lex, want, read.ctc_line_lexicons_read_host(x, lex, nbest, details=True), bar, dist)
    return _cache[name]


def compare_with_spec(name, scores, got, fill=12345.0):
    """what a program made of a case -- scores: (n, >= max count) float64 tensor that was filled with `fill`, got: one LexiconDecoded per
    line parsed from its records -- against the specification: every finite score within the bar, -inf and NaN equal as such, nothing
    written beyond a line's count, the entries in the specification's order (behind margin > 100 x bar, asserted for every line by
    `test_the_seeds_of_the_device_cases_keep_the_margin`) and carrying the program's own scores, flags equal, logz within
    bar + K_b x 2^-52 -> the largest |program - specification| of a finite score"""
    x, lex, want, dec, bar, dist = line_case(name)
    worst = 0.0
    for b, words in enumerate(lex.lists):
        K = len(words)
        row, g, w = scores[b, :K].tolist(), got[b], dec[b]
        assert bool((scores[b, K:] == fill).all()), (name, b)
        if want[b] is None:
            assert all(math.isnan(v) for v in row) and g.entries == [] and g.flag == 1 and math.isnan(g.logz), (name, b, g)
            continue
        for j, (v, s) in enumerate(zip(row, want[b])):
            if s == -math.inf:
                assert v == -math.inf, (name, b, j, v)
            else:
                assert abs(v - s) <= bar, (name, b, j, v, s, bar)
                worst = max(worst, abs(v - s))
        assert w.margin > 100 * bar and g.flag == w.flag == 0, (name, b)
        assert [k for k, _ in g.entries] == [k for k, _ in w.entries], (name, b, g.entries, w.entries)
        assert g.entries == [(k, row[k]) for k, _ in w.entries]      # the entries carry the score buffer's float64 values as they are
        if w.logz == -math.inf:
            assert g.logz == -math.inf, (name, b)
        else:
            assert abs(g.logz - w.logz) <= bar + K * 2.0 ** -52, (name, b, g.logz, w.logz)
    return worst


def corrupt_tables(lex, n):
    """the tables of `lex.pack(range(n))` with corrupt rows among the clean ones, none of which may write anything: tiles whose line,
    segment class, pair range or count is out of range, and a tile of pairs whose union position or j is out of range (j >= the line's
    count on a line with words and on a line without, j beyond the row) -> (tiles, pairs, counts)"""
    tiles, pairs, counts = lex.pack(range(n))
    P, U, most = len(pairs), lex.table.shape[0], int(counts.max())
    empty = [b for b in range(n) if counts[b] == 0]
    extra = [(U, 0), (-1, 1), (0, int(counts[0])), (0, -1), (1, most + 3), (0, 0), (2 ** 30, 2 ** 30)]
    pairs = np.concatenate([pairs, np.asarray(extra, np.int32)])
    bad = [(n, 16, 0, 1), (-1, 16, 0, 1), (0, 16, len(pairs) - 1, 5), (0, 16, -2, 3), (0, 7, 0, 1), (0, 16, 0, 17), (0, 64, 0, 0),
           (0, 32, 2 ** 31 - 4, 8), (0, 16, P, 5), (empty[0] if empty else n, 16, P + 5, 2)]
    tiles = np.concatenate([tiles[:1], np.asarray(bad[:5], np.int32), tiles[1:], np.asarray(bad[5:], np.int32)])
    return tiles, pairs, counts


@pytest.mark.parametrize("name", list(CASES))
def test_every_line_reads_as_it_reads_alone_against_its_list(name):
    from tatt_amd import read
    x, lex, want, dec, bar, dist = line_case(name)
    nbest = CASES[name][5]
    plain = read.ctc_line_lexicons_read_host(x, lex, nbest)
    assert len(dec) == len(plain) == x.shape[1] == len(lex)
    for b, words in enumerate(lex.lists):
        flagged = any(not torch.isfinite(r).any() or torch.isnan(r).any() or (r == math.inf).any() for r in x[:, b])
        if words:
            alone = read.ctc_lexicon_read_host(x[:, b:b + 1], read.Lexicon(words, alphabet=lex.alphabet), nbest, details=True)[0]
            if flagged:
                assert alone.flag == 1 and dec[b].flag == 1 and dec[b].entries == [] and math.isnan(dec[b].logz)
            else:
                assert dec[b] == alone and plain[b] == alone[:3] + (None,)
                assert [v for _, v in dec[b].entries] == [want[b][k] for k, _ in dec[b].entries]
        elif flagged:
            assert plain[b].entries == [] and math.isnan(plain[b].logz) and plain[b].flag == 1
        else:
            assert plain[b] == read.LexiconDecoded([], -math.inf, 0) and dec[b].margin == math.inf


def test_an_empty_list_and_a_flagged_line():
    from tatt_amd import read
    x, _, flags = degenerate_lines()
    got = read.ctc_line_lexicons_read_host(x, read.LineLexicons([[], ["a"], [], ["ab", "a"], ["a"], []], alphabet="-abc"), nbest=2)
    assert got[0] == read.LexiconDecoded([], -math.inf, 0) and got[5] == read.LexiconDecoded([], -math.inf, 0)
    for b in (1, 2, 3):                                              # flagged with and without words
        assert got[b].entries == [] and math.isnan(got[b].logz) and got[b].flag == 1
    assert got[4].flag == 0 and [k for k, _ in got[4].entries] == [0]
    r = read._line_lexicon_reading(got[4], ["a"], 100, False)
    assert r.text == "a" and r.posterior == 1.0 and r.alternatives == [("a", r.logp, 1.0)]
    for g in (got[0], got[1]):
        r = read._line_lexicon_reading(g, [], 120, True)
        assert r.text == "" and math.isnan(r.logp) and r.alternatives == [] and (r.rw, r.squeezed) == (120, True)
    with pytest.raises(ValueError, match="5 lists for 6 lines"):
        read.ctc_line_lexicons_read_host(x, read.LineLexicons([[]] * 5, alphabet="-abc"))
    with pytest.raises(ValueError, match="37 classes"):
        read.ctc_line_lexicons_read_host(x, read.LineLexicons([[]] * 6))
    with pytest.raises(ValueError, match="nbest"):
        read.ctc_line_lexicons_read_host(x, read.LineLexicons([[]] * 6, alphabet="-abc"), nbest=0)


def test_all_strings_against_brute_force():
    x, lex, want, dec, bar, dist = line_case("all-15")
    for b in range(2):
        exact = brute_force(x[:, b])                                 # the 27 alignments, collapsed
        for j, w in enumerate(lex.classes[b]):
            if tuple(w) in exact:
                assert abs(want[b][j] - exact[tuple(w)]) <= 1e-14, (b, w)
            else:
                assert want[b][j] == -math.inf, (b, w)
        feasible = [j for j, w in enumerate(lex.classes[b]) if tuple(w) in exact]
        assert sorted(k for k, _ in dec[b].entries) == feasible
        assert abs(dec[b].logz - math.log(math.fsum(math.exp(exact[tuple(lex.classes[b][j])]) for j in feasible))) <= 1e-14
    assert lex.lists[1] == ["ba", "", "a"] and lex.index[1] == [ALL15.index(w) for w in lex.lists[1]] != [0, 1, 2]   # a word at another j


def test_mapping_and_refusals():
    from tatt_amd import io, read
    lex = read.LineLexicons([["Hello", "a0"], [], ["A0", "", "zz"]])
    assert lex.lists == [["hello", "a0"], [], ["a0", "", "zz"]] and len(lex) == 3 and lex.n_classes == 37 and lex.alphabet == ABC
    assert lex.classes == [[[18, 15, 22, 22, 25], [11, 1]], [], [[11, 1], [], [36, 36]]]
    assert lex.union == ["hello", "a0", "", "zz"] and lex.index == [[0, 1], [], [1, 2, 3]]      # first appearance; one entry per word
    assert len(read.LineLexicons([])) == 0 and read.LineLexicons([]).table.shape == (1, 4)
    for lists, what in (([["ok"], ["ok", "a-b"]], "line 1.*a-b"), ([["café"]], "line 0.*caf"), ([[], [], ["x" * 32]], "line 2.*" + "x" * 32),
                        ([["abc"], ["abc", "ABC"]], "line 1.*'abc'.*twice"), ([["%d" % i for i in range(65537)]], "line 0 has 65537")):
        with pytest.raises(ValueError, match=what):
            read.LineLexicons(lists)
    assert len(read.LineLexicons([["abc"], ["ABC"]]).union) == 1     # the same word on two lines is no duplicate
    with pytest.raises(ValueError):
        read.LineLexicons([["a"]], min_segment=8)
    with pytest.raises(ValueError):
        read.LineLexicons(["abc"])
    with pytest.raises(ValueError):
        read.LineLexicons("abc")
    was = read.LineLexicons.UNION
    try:                                                             # (the limit itself, 2^20 distinct words, is checked by the same line)
        read.LineLexicons.UNION = 3
        assert len(read.LineLexicons([["a", "b"], ["b", "c"]]).union) == 3
        with pytest.raises(ValueError, match="line 1.*'d'.*distinct word 4"):
            read.LineLexicons([["a", "b"], ["b", "c", "d"]])
    finally:
        read.LineLexicons.UNION = was
    assert io.LineLexicons is read.LineLexicons and io.ctc_line_lexicons_read_host is read.ctc_line_lexicons_read_host
    assert io.line_lexicons_limits is read.line_lexicons_limits


def test_packing():
    from tatt_amd import read
    words = ["a" * L + "b" for L in (6, 7, 14, 15, 30)] + ["", "q"]      # lengths 7, 8, 15, 16, 31, 0, 1
    lex = read.LineLexicons([words[3:], words[:4], [], words[::-1]])
    assert lex.union == words[3:] + words[:3]
    assert lex.segments == [read._segment(len(w)) for w in lex.union] == [64, 64, 16, 16, 16, 32, 32]
    assert lex.order == [2, 3, 4, 5, 6, 0, 1] and [lex.packed[u] for u in lex.order] == list(range(7))
    assert lex.table.dtype == np.int32 and lex.table.shape == (7, 4) and lex.table[:, 2].tolist() == lex.order
    for p, u in enumerate(lex.order):
        L, off = int(lex.table[p, 0]), int(lex.table[p, 1])
        assert L == len(lex.union[u]) and lex.table[p, 3] == 0 and 2 * L + 1 <= lex.segments[u]
        assert "".join(lex.alphabet[c] for c in lex.codes[off:off + L]) == lex.union[u]
    assert lex.n_codes == sum(len(w) for w in words) and len(lex.codes) == lex.n_codes + 1
    tiles, pairs, counts = lex.pack([3, 0, 2, 1])                    # a chunk in another order than the input's
    assert tiles.dtype == pairs.dtype == counts.dtype == np.int32 and counts.tolist() == [7, 4, 0, 4]
    assert tiles.tolist() == [[0, 16, 0, 3], [0, 32, 3, 2], [0, 64, 5, 2], [1, 16, 7, 2], [1, 64, 9, 2], [3, 16, 11, 1], [3, 32, 12, 2],
                              [3, 64, 14, 1]]
    _check_pack(lex, [3, 0, 2, 1], tiles, pairs, counts)
    assert read.LineLexicons([words], min_segment=64).pack([0])[0].tolist() == [[0, 64, 0, 4], [0, 64, 4, 3]]
    empty = read.LineLexicons([[], []]).pack([1, 0])
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 2) and empty[2].tolist() == [0, 0]
    for name in CASES:                                               # the device cases: every tile full but the last of its class
        x, big, _ = case_inputs(name)
        lines = list(range(len(big)))[::-1]
        _check_pack(big, lines, *big.pack(lines))
    x, big, _ = case_inputs("reader-T")
    tiles = big.pack(range(5))[0].tolist()
    assert [t[3] for t in tiles if t[0] == 0] == [16, 13, 8, 8, 5] and [t[1:] for t in tiles if t[0] == 1] == [[16, 50, 1]]
    assert [t[3] for t in tiles if t[0] == 3] == [16, 1] and [t[3] for t in tiles if t[0] == 4] == [16] and not [t for t in tiles if t[0] == 2]
    x, big, _ = case_inputs("skew")
    tiles = big.pack(range(4))[0]
    assert (tiles[:, 0] == 1).sum() > 40 and all((tiles[:, 0] == b).sum() <= 3 for b in (0, 2, 3)) and set(tiles[:, 1].tolist()) == {16, 32, 64}


def _check_pack(lex, lines, tiles, pairs, counts):
    """one tile row per non-empty tile, every pair in exactly one tile, G from `_segment`, a line's pairs and its list the same set"""
    from tatt_amd import read
    covered = np.zeros(len(pairs), np.int32)
    for b, G, first, count in tiles.tolist():
        assert 1 <= count <= 256 // G and 0 <= first and first + count <= len(pairs) and 0 <= b < len(lines)
        covered[first:first + count] += 1
        for p, j in pairs[first:first + count].tolist():
            u = lex.order[p]
            assert lex.index[lines[b]][j] == u and read._segment(len(lex.union[u]), lex.min_segment) == G == lex.segments[u]
            assert int(lex.table[p, 0]) == len(lex.union[u])
    assert bool((covered == 1).all())
    assert counts.tolist() == [len(lex.lists[i]) for i in lines] and len(pairs) == int(counts.sum())
    for b, i in enumerate(lines):
        mine = [pairs[f + k].tolist() for bb, G, f, c in tiles.tolist() if bb == b for k in range(c)]
        assert sorted(j for _, j in mine) == list(range(len(lex.lists[i])))
        assert {lex.union[lex.order[p]] for p, _ in mine} == set(lex.lists[i])
    full = {}
    for b, G, first, count in tiles.tolist():                        # no empty work-groups, and only a class's last tile is short
        full.setdefault((b, G), []).append(count)
    assert all(c == 256 // G for (b, G), cs in full.items() for c in cs[:-1])


def test_limits_header_and_refusals():
    from tatt_amd import read
    from tatt_amd._lib import LIB, parse_header
    from tatt_amd.build import SOURCES
    lim = read.line_lexicons_limits()
    assert lim == {"steps": 256, "classes": 64, "length": 31, "words": 65536, "union": 1048576, "nbest": 16}
    assert {k: v for k, v in lim.items() if k != "union"} == read.lexicon_limits() and read.LineLexicons.UNION == lim["union"]
    assert "ctclexp.hip" in SOURCES
    protos = parse_header()
    for name in ("tatt_ctc_lexicon_score_pairs", "tatt_ctc_lexicon_select_rows", "tatt_line_lexicons_limits"):
        assert name in protos and getattr(LIB, name) is not None, name
    assert [n for _, n in protos["tatt_ctc_lexicon_score_pairs"]] == [
        "logits", "st_t", "st_b", "st_c", "T", "B", "C", "codes", "n_codes", "words", "U", "tiles", "n_tiles", "pairs", "n_pairs", "counts",
        "max_count", "scores", "st_sc", "st"]
    assert [n for _, n in protos["tatt_ctc_lexicon_select_rows"]] == ["scores", "st_sc", "B", "counts", "nbest", "index", "record", "n_rows",
                                                                      "st_rec", "st"]
    # null pointers and bad sizes: 1, before any launch (nothing here touches a device)
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    score = dict(logits=p, codes=p, words=p, tiles=p, pairs=p, counts=p, scores=p, T=26, B=2, C=37, n_codes=3, U=2, n_tiles=1, n_pairs=2,
                 max_count=2, st_sc=2)

    def run_score(a):
        return LIB.tatt_ctc_lexicon_score_pairs(a["logits"], 74, 37, 1, a["T"], a["B"], a["C"], a["codes"], a["n_codes"], a["words"], a["U"],
                                                a["tiles"], a["n_tiles"], a["pairs"], a["n_pairs"], a["counts"], a["max_count"], a["scores"],
                                                a["st_sc"], None)
    assert LIB.tatt_line_lexicons_limits(None) == 1
    for kw in ({"logits": None}, {"codes": None}, {"words": None}, {"tiles": None}, {"pairs": None}, {"counts": None}, {"scores": None},
               {"T": 0}, {"T": 257}, {"C": 0}, {"C": 65}, {"B": 0}, {"B": 65536}, {"U": 0}, {"U": 1048577}, {"n_codes": -1}, {"n_tiles": 0},
               {"n_tiles": -1}, {"n_pairs": 0}, {"n_pairs": -2}, {"n_tiles": 3}, {"max_count": 0}, {"max_count": 65537, "st_sc": 65537},
               {"st_sc": 1}, {"st_sc": -1}):
        assert run_score(dict(score, **kw)) == 1, kw
    select = dict(scores=p, counts=p, index=p, record=p, st_sc=2, B=1, nbest=4, n_rows=1, st_rec=20)
    for kw in ({"scores": None}, {"counts": None}, {"index": None}, {"record": None}, {"B": 0}, {"st_sc": 0}, {"st_sc": -3}, {"nbest": 0},
               {"nbest": 17}, {"n_rows": 0}, {"st_rec": 19}):
        a = dict(select, **kw)
        assert LIB.tatt_ctc_lexicon_select_rows(a["scores"], a["st_sc"], a["B"], a["counts"], a["nbest"], a["index"], a["record"],
                                                a["n_rows"], a["st_rec"], None) == 1, kw
    cpu = torch.zeros(2, 1, 37)
    i32 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        read.ctc_lexicon_score_pairs(cpu, i32, 0, i32.view(1, 4), i32.view(1, 4), i32.view(2, 2), i32[:1], torch.zeros(1, 2, dtype=torch.float64), 2)
    with pytest.raises(RuntimeError):
        read.ctc_lexicon_select_rows(torch.zeros(1, 2, dtype=torch.float64), i32[:1], i32[:1], torch.zeros(1, 20, dtype=torch.int32))


def test_the_reader_refuses_before_it_looks_at_a_device():
    import tatt_amd
    from tatt_amd import read
    module = torch.nn.Linear(1, 1)                                   # the keywords are checked before the module is looked at
    with pytest.raises(ValueError, match="lexicon="):
        read.LineReader(module, decode="lexicons", lexicon=["a"])
    with pytest.raises(ValueError, match="lexicon="):
        read.LineReader(module, decode="lexicon")                    # (as before)
    for nbest in (0, 17, 4.0):
        with pytest.raises(ValueError, match="nbest <= 16"):
            read.LineReader(module, decode="lexicons", nbest=nbest)
    with pytest.raises(ValueError, match="word_penalty"):
        read.LineReader(module, decode="lexicons", word_penalty=1.0)
    with pytest.raises(ValueError, match="lm="):
        read.LineReader(module, decode="lexicons", lm=read.CharLM.from_corpus(["ab"], order=2))
    with pytest.raises(ValueError, match="'lexicons'"):
        read.LineReader(module, decode="dictionary")
    reader = object.__new__(read.LineReader)                         # the call's own checks touch no device: run them without one
    reader.decode, reader.crnn = "lexicons", tatt_amd.CRNN(32, 1, 37, 8)
    got = reader.check_lexicons([["a"], []], 2)
    assert isinstance(got, read.LineLexicons) and got.lists == [["a"], []] and reader.check_lexicons(got, 2) is got
    with pytest.raises(ValueError, match="needs lexicons="):
        reader.check_lexicons(None, 2)
    with pytest.raises(ValueError, match="2 lists of words for 3 lines"):
        reader.check_lexicons([["a"], []], 3)
    with pytest.raises(ValueError, match="emits 37"):
        reader.check_lexicons(read.LineLexicons([["a"]], alphabet=ABC64), 1)
    with pytest.raises(ValueError, match="twice"):
        reader.check_lexicons([["a", "A"]], 1)
    for decode in ("greedy", "beam", "lexicon", "words"):
        reader.decode = decode
        assert reader.check_lexicons(None, 2) is None
        with pytest.raises(ValueError, match="decode='lexicons'"):
            reader.check_lexicons([["a"], []], 2)


@pytest.mark.parametrize("name", list(CASES))
def test_the_seeds_of_the_device_cases_keep_the_margin(name):
    """the device test asserts the ORDER of a line's entries only behind margin > 100 x bar, and no line may be left out"""
    T, n, C, alphabet, lists, nbest, seed = CASES[name]
    x, lex, want, dec, bar, dist = line_case(name)
    assert tuple(x.shape) == (T, n, C) and lex.n_classes == C and len(dec) == n == len(lex) and [len(w) for w in lex.lists] == [len(w) for w in lists]
    gap = min(d.margin for d in dec)
    print("%s: bar %.3g (float64 - longdouble %.3g), smallest neighbour gap %.3g, entries %s" % (name, bar, dist, gap,
                                                                                                [len(d.entries) for d in dec]))
    for b, d in enumerate(dec):
        assert d.margin > 100 * bar, (name, b, d.margin, bar)
        if want[b] is not None:
            assert d.flag == 0 and len(d.entries) == min(nbest, sum(v > -math.inf for v in want[b]))
    if name == "reader-T":
        assert [len(w) for w in lists] == [50, 1, 0, 17, 16] and {len(w) for ws in lists for w in ws} == set(range(1, 13))
        shared = [sum(w in lists[0] for w in ws) for ws in lists]
        assert shared[3:] == [9, 8] and lists[1][0] in lists[0]      # half the words of the short lists are line 0's
    if name == "skew":
        assert [len(w) for w in lists] == [3, 300, 3, 3] and max(len(w) for w in lists[1]) == 31
        assert sum(any(a == b for a, b in zip(w, w[1:])) for w in lists[1]) >= 8 and all(v > -math.inf for v in want[1])
    if name == "degenerate":
        assert [d.flag for d in dec] == [0, 1, 1, 1, 0, 0] and dec[5].entries == [] and dec[5].logz == -math.inf
