"""The beam search with a character n-gram language model on the host (tatt_amd/read.py: CharLM, char_lm_score_host,
ctc_beam_lm_read_host, parse_beam_lm_records), the specification of tatt_ctc_beam_lm_read in csrc/ctcbeam.hip.  Yardstick: brute force over
all C^T alignments (tests/test_beam.brute_force) with the LM term of every string summed by char_lm_score_host, where a beam is wide enough
to keep every string; the plain search where the table is all zeros; values written out by hand.  No GPU."""
import math
import struct

import numpy as np
import pytest
import torch

from tests.test_beam import CASES, REENTRY, beam_case, beam_logits, brute_force

# (T, B, C, beam, nbest, order, s, weight, bonus, seed): the shapes tests/test_beam_lm_device_gpu.py runs on the device.  The seeds are
# chosen on the CPU so that the specification ALONE has, on every row, a margin above 100 x (bar + 2^-52 max |score|)
# (test_the_seeded_cases_leave_a_margin), and so that the last shape has a row with a re-entry under the fused specification.
LM_CASES = ((1, 1, 2, 1, 1, 1, 3.0, .5, 0.0, 11), (3, 2, 3, 16, 16, 3, 3.0, .5, 0.0, 12), (26, 3, 37, 8, 4, 3, 3.0, .5, 0.0, 13),
            (26, 3, 37, 8, 4, 2, 3.0, 1.0, 0.7, 13), (64, 17, 37, 5, 5, 3, 3.0, .5, 0.0, 14), (256, 2, 37, 16, 4, 3, 3.0, .5, 0.0, 15),
            (7, 1, 64, 16, 1, 3, 3.0, .5, 0.0, 16), (40, 16, 5, 4, 4, 2, 2.0, .3, 0.0, 18))
LM_REENTRY = LM_CASES[-1]
_cache, _tables = {}, {}


def lm_table(C, order, seed):
    """log_softmax(randn * 2) of shape (C,) * order from a fixed seed -> CharLM (one per geometry, shared)"""
    from tatt_amd import read
    key = (C, order, seed)
    if key not in _tables:
        g = torch.Generator().manual_seed(1000 + seed)
        _tables[key] = read.CharLM(torch.log_softmax(torch.randn((C,) * order, generator=g, dtype=torch.float64) * 2, -1).numpy())
    return _tables[key]


def lm_case(case):
    """-> (logits, CharLM, the specification's result with details); computed once and shared, never changed"""
    if case not in _cache:
        from tatt_amd import read
        T, B, C, beam, nbest, order, s, weight, bonus, seed = case
        x, lm = beam_logits(T, B, C, s, seed), lm_table(C, order, seed)
        _cache[case] = (x, lm, read.ctc_beam_lm_read_host(x, lm, beam, nbest, weight, bonus, details=True))
    return _cache[case]


def lm_bar(case):
    """-> (the bar on logp, the distance float64 - longdouble of the specification, 2^-52 max |score|) of a case, from the specification
    alone; strings must agree between the two runs"""
    key = ("bar", case)
    if key not in _cache:
        from tatt_amd import read
        T, B, C, beam, nbest, order, s, weight, bonus, seed = case
        x, lm, want = lm_case(case)
        wide = read.ctc_beam_lm_read_host(x, lm, beam, nbest, weight, bonus, real=np.longdouble)
        dist = top = score = 0.0
        for w, l in zip(want, wide):
            assert [c for c, _, _ in w.entries] == [c for c, _, _ in l.entries]
            assert [m for _, _, m in w.entries] == [m for _, _, m in l.entries]          # (the LM term is float64 under both settings)
            dist = max(dist, max(abs(float(np.longdouble(a[1]) - b[1])) for a, b in zip(w.entries, l.entries)))
            top = max(top, max(abs(a[1]) for a in w.entries))
            score = max(score, max(abs(a[1] + a[2]) for a in w.entries))
        _cache[key] = (4 * dist + T * 2.0 ** -52 * top, dist, 2.0 ** -52 * score)
    return _cache[key]


def test_char_lm_refusals():
    from tatt_amd import io, read
    ok = np.log(np.full((3, 3), 1 / 3))
    assert (read.CharLM(ok).order, read.CharLM(ok).n_classes, read.CharLM(ok[0]).order) == (2, 3, 1)
    for bad in (np.zeros((3, 4)), np.zeros(()), np.zeros((2, 2, 2, 2)), np.zeros((1,)), np.zeros((65, 65)), np.zeros((3, 3, 2))):
        with pytest.raises(ValueError):
            read.CharLM(bad)
    for v in (-math.inf, math.inf, math.nan):
        t = ok.copy()
        t[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            read.CharLM(t)
    with pytest.raises(ValueError, match="alphabet"):
        read.CharLM(ok, alphabet="-abc")
    assert read.CharLM(ok, alphabet="-ab").alphabet == "-ab" and read.CharLM(np.zeros((37,))).alphabet == "-" + io.ALPHABET
    assert read.lm_limits() == {"order": 3, "classes": 64} == {"order": read.CharLM.ORDER, "classes": read.CharLM.CLASSES}
    assert read.lm_limits()["classes"] == read.beam_limits()["classes"]
    lm = read.CharLM(ok)
    for kw in ({"weight": math.inf}, {"bonus": math.nan}, {"weight": "much"}, {"weight": 1e308, "bonus": -1e308}, {"weight": 1e306},
               {"bonus": -1e306}):                                   # (the last two: finite entries whose sum over a line is not)
        with pytest.raises(ValueError):
            lm.increments(**{"weight": .5, "bonus": 0.0, **kw})
    x = beam_logits(3, 1, 3, 3.0, 50)
    for kw in ({"beam": 0, "nbest": 0}, {"beam": 4, "nbest": 5}):
        with pytest.raises(ValueError):
            read.ctc_beam_lm_read_host(x, lm, **kw)
    with pytest.raises(ValueError, match="classes"):
        read.ctc_beam_lm_read_host(beam_logits(3, 1, 4, 3.0, 50), lm)
    with pytest.raises(ValueError):
        read.ctc_beam_lm_read_host(x, ok)
    assert io.CharLM is read.CharLM and io.ctc_beam_lm_read_host is read.ctc_beam_lm_read_host and io.lm_limits is read.lm_limits
    assert io.BeamLMReading is read.BeamLMReading and io.char_lm_score_host is read.char_lm_score_host
    module = torch.nn.Linear(1, 1)                                   # the keywords are checked before the module is looked at
    assert abs(lm.increments(1e300, -1e300)).max() * 257 < math.inf
    for kw in ({"decode": "greedy", "lm": lm}, {"decode": "lexicon", "lexicon": ["a"], "lm": lm}, {"decode": "beam", "lm_weight": .5},
               {"decode": "beam", "lm_bonus": 0.0}, {"decode": "greedy", "lm_weight": .5}, {"decode": "beam", "lm": ok},
               {"decode": "beam", "lm": lm, "lm_weight": math.inf}):
        with pytest.raises(ValueError, match="lm"):
            read.LineReader(module, **kw)


def test_increments_table():
    from tatt_amd import read
    lm = lm_table(5, 3, 1)
    W = lm.increments(0.3, 0.7)
    assert W.shape == (5, 5, 5) and W.dtype == np.float64 and W.flags["C_CONTIGUOUS"]
    assert (W[..., 1:] == 0.3 * lm.logp[..., 1:] + 0.7).all() and (W[..., 0] == 0.3 * lm.logp[..., 0]).all()
    chars, end = read.char_lm_score_host(W, [2, 4, 4, 1])
    assert chars == (((0.0 + W[0, 0, 2]) + W[0, 2, 4]) + W[2, 4, 4]) + W[4, 4, 1] and end == W[4, 1, 0]
    assert read.char_lm_score_host(W, []) == (0.0, W[0, 0, 0])
    W2, W1 = lm_table(5, 2, 1).increments(1.0, 0.0), lm_table(5, 1, 1).increments(1.0, 0.0)
    assert read.char_lm_score_host(W2, [3, 1]) == ((0.0 + W2[0, 3]) + W2[3, 1], W2[1, 0])
    assert read.char_lm_score_host(W1, [3, 1]) == ((0.0 + W1[3]) + W1[1], W1[0])
    with pytest.raises(ValueError):
        read.char_lm_score_host(W, [5])
    with pytest.raises(ValueError):
        read.char_lm_score_host(W, [0])


def test_from_corpus():
    from tatt_amd import read
    lm = read.CharLM.from_corpus(["ab", "ab", "b"], order=2, alphabet="-ab", smoothing=1)
    # unigrams: end 3, a 2, b 3 of 8 events: P_1 = (count + 1/3) / 9 = (10, 7, 10) / 27
    # after the begin: a 2, b 1: (count + P_1) / 4; after a: b 2: / 3; after b: end 3: / 4
    want = [[10 / 108, 61 / 108, 37 / 108], [10 / 81, 7 / 81, 64 / 81], [91 / 108, 7 / 108, 10 / 108]]
    assert np.abs(np.exp(lm.logp) - np.asarray(want)).max() <= 1e-15 and lm.order == 2 and lm.alphabet == "-ab"
    uni = read.CharLM.from_corpus(["ab", "ab", "b"], order=1, alphabet="-ab")
    assert np.abs(np.exp(uni.logp) - np.asarray([10 / 27, 7 / 27, 10 / 27])).max() <= 1e-15
    corpus = ["Main St", "exit 12", "OPEN", "open", "a", ""]
    corpus = [s.replace(" ", "") for s in corpus]
    for order in (1, 2, 3):
        a = read.CharLM.from_corpus(corpus, order=order)
        assert a.logp.shape == (37,) * order and np.abs(np.exp(a.logp).sum(-1) - 1.0).max() <= 1e-12
        b = read.CharLM.from_corpus([s.lower() for s in corpus], order=order)
        assert a.logp.tobytes() == b.logp.tobytes()                  # lower-casing, and the same bits from the same corpus
    with pytest.raises(ValueError, match="'exit 12'"):
        read.CharLM.from_corpus(["open", "exit 12"])
    for kw in ({"order": 4}, {"order": 0}, {"smoothing": 0.0}, {"smoothing": math.inf}, {"alphabet": "-"}):
        with pytest.raises(ValueError):
            read.CharLM.from_corpus(["a"], **kw)
    with pytest.raises(ValueError):
        read.CharLM.from_corpus("open")


@pytest.mark.parametrize("T,C,strings", ((3, 3, 9), (4, 3, 15)))
@pytest.mark.parametrize("order", (1, 2, 3))
def test_an_exhaustive_fused_beam_equals_brute_force(T, C, strings, order):
    from tatt_amd import read
    x, lm = beam_logits(T, 2, C, 3.0, 20 + T), lm_table(C, order, 20 + T)
    W = lm.increments(0.5, 0.0)
    got = read.ctc_beam_lm_read_host(x, lm, beam=16, nbest=16)
    for b, g in enumerate(got):
        rows = [(k, v) + read.char_lm_score_host(W, k) for k, v in brute_force(x[:, b]).items()]
        rows.sort(key=lambda e: -((e[1] + e[2]) + e[3]))
        assert len(rows) == strings and g.flag == 0
        assert [tuple(c) for c, _, _ in g.entries] == [k for k, _, _, _ in rows], (b, g.entries, rows)
        assert max(abs(a[1] - w[1]) for a, w in zip(g.entries, rows)) <= 1e-14
        assert all(struct.pack("<d", a[2]) == struct.pack("<d", w[2] + w[3]) for a, w in zip(g.entries, rows))


@pytest.mark.parametrize("case", (CASES[2], REENTRY), ids=("T26", "re-entry"))
def test_a_zero_weight_is_the_plain_search(case):
    from tatt_amd import read
    T, B, C, beam, nbest, s, seed = case
    x, want = beam_case(case)
    got = read.ctc_beam_lm_read_host(x, lm_table(C, 3, seed), beam, nbest, weight=0, bonus=0, details=True)
    for g, w in zip(got, want):
        assert [(c, lg) for c, lg, _ in g.entries] == w.entries and all(m == 0.0 for _, _, m in g.entries)
        assert (g.flag, g.margin, g.reentry, g.reranked) == (0, w.margin, w.reentry, False)


def planted_line():
    """-> (logits (5, 1, 37) whose acoustics put "cot" slightly above "cat", the model of a corpus that has seen "cat" twenty times)"""
    from tatt_amd import read
    abc = "-0123456789abcdefghijklmnopqrstuvwxyz"
    x = torch.full((5, 1, 37), -6.0)
    for t, ch in enumerate("c-?-t"):
        if ch == "?":
            x[t, 0, abc.index("o")], x[t, 0, abc.index("a")] = 4.0, 3.8
        else:
            x[t, 0, abc.index(ch)] = 4.0
    return x, read.CharLM.from_corpus(["cat"] * 20 + ["cot"])


def test_the_model_decides_a_planted_line():
    from tatt_amd import read
    x, lm = planted_line()
    abc = "-0123456789abcdefghijklmnopqrstuvwxyz"

    def text(d):
        return "".join(abc[c] for c in d.entries[0][0])
    assert text(read.ctc_beam_read_host(x, 8, 4)[0]) == "cot"
    fused = read.ctc_beam_lm_read_host(x, lm, 8, 4)[0]
    assert text(fused) == "cat" and "".join(abc[c] for c in fused.entries[1][0]) == "cot"
    assert fused.entries[0][1] < fused.entries[1][1] and fused.entries[0][2] > fused.entries[1][2]     # less mass, more prior
    assert text(read.ctc_beam_lm_read_host(x, lm, 8, 4, weight=0)[0]) == "cot"


@pytest.mark.parametrize("case", LM_CASES, ids=lambda c: "T%d-B%d-C%d-beam%d-order%d" % (c[:4] + c[5:6]))
def test_the_seeded_cases_leave_a_margin(case):
    """what tests/test_beam_lm_device_gpu.py asserts of every row before it compares: stated here on the specification alone"""
    T, B, C, beam, nbest, order, s, weight, bonus, seed = case
    x, lm, want = lm_case(case)
    bar, dist, ulp = lm_bar(case)
    print("case %s: bar %.3g, smallest margin %.3g, rows with a re-entry %d, re-ranked %d"
          % (case[:9], bar, min(w.margin for w in want), sum(w.reentry for w in want), sum(w.reranked for w in want)))
    W = lm.increments(weight, bonus)
    for b, w in enumerate(want):
        assert w.flag == 0 and 1 <= len(w.entries) <= nbest
        assert w.margin > 100 * (bar + ulp), "row %d: margin %.3g against %.3g: take another seed" % (b, w.margin, 100 * (bar + ulp))
        finals = [lg + m for _, lg, m in w.entries]
        assert all(a >= b_ for a, b_ in zip(finals, finals[1:])) and len({tuple(c) for c, _, _ in w.entries}) == len(w.entries)
        for c, lg, m in w.entries:
            chars, end = read_score(W, c)
            assert struct.pack("<d", m) == struct.pack("<d", chars + end)
            assert lg <= exact_logp(x[:, b], c) + 1e-9
    if case is LM_REENTRY:
        assert any(w.reentry for w in want)


def read_score(W, classes):
    from tatt_amd import read
    return read.char_lm_score_host(W, classes)


def exact_logp(row, classes):
    from tatt_amd import read
    return read.ctc_string_logp_host(row, classes)


def test_a_bonus_never_shortens_the_best_string():
    """on the seeded cases (and on them only: it is no theorem of a pruned search)"""
    from tatt_amd import read
    for case in LM_CASES:
        T, B, C, beam, nbest, order, s, weight, bonus, seed = case
        x, lm, want = lm_case(case)
        more = read.ctc_beam_lm_read_host(x, lm, beam, nbest, weight, bonus + 1.0)
        assert all(len(m.entries[0][0]) >= len(w.entries[0][0]) for m, w in zip(more, want)), case


def test_the_end_term_re_ranks():
    """a seeded case has rows whose order the end term changes; and a table whose end column is chosen so that it must"""
    from tatt_amd import read
    assert any(w.reranked for case in LM_CASES[1:4] for w in lm_case(case)[2])
    x = beam_logits(4, 1, 3, 3.0, 24)
    plain = read.ctc_beam_lm_read_host(x, read.CharLM(np.zeros((3, 3))), 16, 16, details=True)[0]
    assert not plain.reranked
    t = np.zeros((3, 3))
    t[2, 0] = 200.0                                                  # a line that ends after class 2 wins by far
    got = read.ctc_beam_lm_read_host(x, read.CharLM(t), 16, 16, weight=1.0, details=True)[0]
    was = [c for c, _, _ in plain.entries]
    first, rest = [c for c in was if c[-1:] == [2]], [c for c in was if c[-1:] != [2]]
    assert first and rest and was != first + rest and got.reranked
    assert [c for c, _, _ in got.entries] == first + rest            # (ties of a rounded sum go to the lower rank: a stable partition)
    assert [m for _, _, m in got.entries] == [200.0] * len(first) + [0.0] * len(rest)
    assert sorted((c, lg) for c, lg, _ in got.entries) == sorted((c, lg) for c, lg, _ in plain.entries)


def tie_tables():
    """-> [(CharLM over 4 classes, the order of the 5 best strings of all-equal (2, 1, 4) logits at weight 1, their LM terms)], by hand.
    A table of zeros: the plain search's order (tests/test_beam.py has it by hand).  A table that prefers class 2 and dislikes class 1 by
    exact amounts: step 1 keeps 2 (0.5), then the stay candidate and 3 (0, keys 0 and 3), then 1 (-0.25); step 2 ranks by mass + term:
    2 (log 3/16 + 0.5), 3 (log 3/16), 1 (log 3/16 - 0.25), then the strings of mass log 1/16: 23 and 32 (0.5 each; the beam was 2, "",
    3, 1, so their keys are 0 C + 3 and 2 C + 2: 23 first)."""
    from tatt_amd import read
    return [(read.CharLM(np.zeros((4, 4, 4))), [[1], [2], [3], [], [1, 2]], [0.0] * 5),
            (read.CharLM(np.asarray([0.0, -0.25, 0.5, 0.0])), [[2], [3], [1], [2, 3], [3, 2]], [0.5, 0.0, -0.25, 0.5, 0.5])]


def flagged_lines():
    """(6, 6, 4) logits: a clean line, a NaN, a +inf, a line without the blank and class 2, a line of the blank and 3 only (a beam shorter
    than `beam`), a step without a finite logit -> (logits, the flags)"""
    inf = float("inf")
    x = beam_logits(6, 6, 4, 3.0, 40)
    x[2, 1, 3] = float("nan")
    x[5, 2, 0] = inf
    x[:, 3, 0] = -inf
    x[:, 3, 2] = -inf
    x[:, 4, 1:3] = -inf
    x[3, 5] = -inf
    return x, [0, 1, 1, 0, 0, 1]


def test_exact_ties():
    from tatt_amd import read
    x = torch.zeros(2, 1, 4)
    (zero_lm, zero_order, zero_terms), (lm, order, terms) = tie_tables()
    zero = read.ctc_beam_lm_read_host(x, zero_lm, 5, 5, weight=1.0, details=True)[0]
    assert [c for c, _, _ in zero.entries] == zero_order and zero.margin == 0.0 and not zero.reranked
    assert [m for _, _, m in zero.entries] == zero_terms
    plain = read.ctc_beam_read_host(x, 5, 5)[0]
    assert [(c, lg) for c, lg, _ in zero.entries] == plain.entries
    got = read.ctc_beam_lm_read_host(x, lm, 5, 5, weight=1.0, details=True)[0]
    assert [c for c, _, _ in got.entries] == order, got.entries
    assert [m for _, _, m in got.entries] == terms
    assert got.entries[0][1] == got.entries[1][1] == got.entries[2][1] and got.entries[3][1] == got.entries[4][1]


def test_flagged_lines():
    from tatt_amd import read
    x, flags = flagged_lines()
    got = read.ctc_beam_lm_read_host(x, lm_table(4, 2, 40), 8, 8, details=True)
    assert [g.flag for g in got] == flags and [len(g.entries) for g in got] == [8, 0, 0, 8, 4, 0]
    assert got[1] == read.BeamLMDecoded([], 1, math.inf, False, False)
    assert read.ctc_beam_lm_read_host(x[:, 1:2], lm_table(4, 2, 40))[0] == read.BeamLMDecoded([], 1)


def test_record_round_trip():
    from tatt_amd import read
    cap, nbest = 5, 3
    es = read.beam_lm_entry_words(cap)
    assert es == 12 and read.beam_lm_record_words(cap, nbest) == 38 and read.beam_lm_entry_words(6) == 12

    def entry(logp, lm, classes):
        return list(struct.unpack("<iiii", struct.pack("<dd", logp, lm))) + [len(classes), 0] + classes + [-1] * (es - 6 - len(classes))
    a, m = -0.1234567890123456789, -3.0000000000000004               # (not representable in fp32: the float64s travel as they are)
    rows = [[2, 0] + entry(a, m, [3, 1, 36]) + entry(-7.5, 0.25, []) + [-77] * es + [-77] * 3,
            [0, 1] + [-77] * (3 * es + 3),
            [3, 0] + entry(0.0, -0.0, [1, 2, 3, 4, 5]) + entry(-1e-300, 1e-300, [9]) + entry(-745.5, -2.5, [2, 2]) + [-77] * 3]
    got = read.parse_beam_lm_records(torch.tensor(rows, dtype=torch.int32), cap, nbest)
    assert got[0] == read.BeamLMDecoded([([3, 1, 36], a, m), ([], -7.5, 0.25)], 0)
    assert got[1] == read.BeamLMDecoded([], 1)
    assert got[2] == read.BeamLMDecoded([([1, 2, 3, 4, 5], 0.0, -0.0), ([9], -1e-300, 1e-300), ([2, 2], -745.5, -2.5)], 0)
    r = read._beam_lm_reading(got[0], 120, False)
    assert r == read.BeamLMReading("20z", a, m, a + m, [("20z", a, m), ("", -7.5, 0.25)], 120, False)
    f = read._beam_lm_reading(got[1], 100, True)
    assert f.text == "" and math.isnan(f.logp) and math.isnan(f.lm) and math.isnan(f.score) and f.alternatives == [] and f.squeezed
    with pytest.raises(ValueError):
        read.parse_beam_lm_records(torch.tensor([[4, 0] + [0] * 36], dtype=torch.int32), cap, nbest)
