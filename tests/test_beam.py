"""The CTC prefix beam search on the host (tatt_amd/read.py: ctc_beam_read_host, ctc_string_logp_host, parse_beam_records), the
specification of csrc/ctcbeam.hip.  Yardstick: brute force over all C^T alignments where that is possible (a beam wide enough to keep every
string), the exact forward recursion as an upper bound elsewhere.  No GPU."""
import itertools
import math
import struct

import pytest
import torch

# (T, B, C, beam, nbest, s, seed): the shapes tests/test_beam_device_gpu.py runs on the device
CASES = ((1, 1, 2, 1, 1, 3.0, 11), (3, 2, 3, 16, 16, 3.0, 12), (26, 3, 37, 8, 4, 3.0, 13), (64, 17, 37, 5, 5, 3.0, 14),
         (256, 2, 37, 16, 4, 3.0, 15), (7, 1, 64, 16, 1, 3.0, 16), (26, 8, 37, 8, 4, 8.0, 17), (40, 16, 5, 4, 4, 2.0, 18))
REENTRY = CASES[-1]
_cache = {}


def beam_logits(T, B, C, s, seed):
    """randn * s from a fixed seed, fp32"""
    return (torch.randn(T, B, C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * s).to(torch.float32)


def beam_case(case):
    """-> (logits, the specification's result with details); computed once and shared, never changed"""
    if case not in _cache:
        from tatt_amd import read
        T, B, C, beam, nbest, s, seed = case
        x = beam_logits(T, B, C, s, seed)
        _cache[case] = (x, read.ctc_beam_read_host(x, beam, nbest, details=True))
    return _cache[case]


def brute_force(row):
    """row: (T, C) logits -> {string: log-probability}: every alignment's probability from a float64 log-soft-max, summed per collapsed
    string with math.fsum"""
    lp = torch.log_softmax(row.double(), -1).tolist()
    T, C = len(lp), len(lp[0])
    mass = {}
    for path in itertools.product(range(C), repeat=T):
        string = tuple(c for i, c in enumerate(path) if c != 0 and (i == 0 or c != path[i - 1]))
        mass.setdefault(string, []).append(math.exp(sum(lp[t][c] for t, c in enumerate(path))))
    return {k: math.log(m) for k, m in ((k, math.fsum(v)) for k, v in mass.items()) if m > 0.0}


@pytest.mark.parametrize("T,C,strings", ((3, 3, 9), (4, 3, 15)))
def test_an_exhaustive_beam_equals_brute_force(T, C, strings):
    from tatt_amd import read
    x = beam_logits(T, 2, C, 3.0, 20 + T)
    got = read.ctc_beam_read_host(x, beam=16, nbest=16)
    worst = 0.0
    for b, g in enumerate(got):
        want = sorted(brute_force(x[:, b]).items(), key=lambda kv: -kv[1])
        assert len(want) == strings and g.flag == 0
        assert [tuple(c) for c, _ in g.entries] == [k for k, _ in want], (b, g.entries, want)
        worst = max(worst, max(abs(lg - w) for (_, lg), (_, w) in zip(g.entries, want)))
        for k, w in want:                                            # and the forward recursion gives the same numbers
            assert abs(read.ctc_string_logp_host(x[:, b], k) - w) <= 1e-14, (b, k)
    print("T %d C %d: max |logp - brute force| = %.3g" % (T, C, worst))
    assert worst <= 1e-14


def test_string_logp_of_strings_no_alignment_spells():
    from tatt_amd import read
    x = beam_logits(3, 1, 4, 3.0, 30)[:, 0]
    assert read.ctc_string_logp_host(x, [1, 2, 3]) > -math.inf
    assert read.ctc_string_logp_host(x, [1, 1]) > -math.inf          # 1 - 1 needs all three steps
    assert read.ctc_string_logp_host(x, [1, 1, 2]) == -math.inf and read.ctc_string_logp_host(x, [1, 2, 3, 1]) == -math.inf
    total = math.fsum(math.exp(v) for v in brute_force(x).values())
    assert abs(total - 1.0) <= 1e-12
    with pytest.raises(ValueError):
        read.ctc_string_logp_host(x, [4])
    with pytest.raises(ValueError):
        read.ctc_string_logp_host(x, [0])
    with pytest.raises(ValueError):
        read.ctc_string_logp_host(x.reshape(3, 1, 4), [1])
    y = x.clone()
    y[1, 2] = float("nan")
    assert math.isnan(read.ctc_string_logp_host(y, [1]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-B%d-C%d-beam%d" % c[:4])
def test_a_beam_sums_a_subset_of_the_strings_alignments(case):
    """every returned logp <= the exact log-probability of its string + 1e-9; entries are distinct strings in descending order"""
    from tatt_amd import read
    T, B, C, beam, nbest, s, seed = case
    x, want = beam_case(case)
    gap = math.inf
    for b, w in enumerate(want):
        assert w.flag == 0 and 1 <= len(w.entries) <= nbest and w.margin > 0
        strings = [tuple(c) for c, _ in w.entries]
        assert len(set(strings)) == len(strings) and all(len(k) <= T and all(1 <= c < C for c in k) for k in strings)
        assert all(a[1] >= b_[1] for a, b_ in zip(w.entries, w.entries[1:]))
        for classes, logp in w.entries:
            exact = read.ctc_string_logp_host(x[:, b], classes)
            assert logp <= exact + 1e-9, (b, classes, logp, exact)
            gap = min(gap, exact - logp)
    plain = read.ctc_beam_read_host(x, beam, nbest)
    assert [(p.entries, p.flag) for p in plain] == [(w.entries, w.flag) for w in want] and plain[0].margin is None
    print("smallest margin %.3g, smallest exact - beam %.3g" % (min(w.margin for w in want), gap))


def test_the_reentry_shape_has_rows_that_re_enter():
    """without such a row the device test of this shape says nothing about the identity of trie nodes"""
    _, want = beam_case(REENTRY)
    rows = [b for b, w in enumerate(want) if w.reentry]
    print("rows with a re-entry: %s" % rows)
    assert len(rows) >= 1
    assert not any(w.reentry for w in beam_case(CASES[0])[1])


def test_flagged_lines_and_inf_columns():
    from tatt_amd import read
    x = beam_logits(6, 5, 4, 3.0, 40)
    x[2, 1, 3] = float("nan")
    x[5, 2, 0] = float("inf")
    x[:, 3, 0] = -float("inf")                                       # no blank, classes 1 and 3 only
    x[:, 3, 2] = -float("inf")
    x[:, 4, 1:3] = -float("inf")                                     # blank and 3: a handful of strings
    got = read.ctc_beam_read_host(x, beam=8, nbest=8, details=True)
    assert got[0].flag == 0 and len(got[0].entries) == 8
    assert got[1] == read.BeamDecoded([], 1, math.inf, False) and got[2].entries == [] and got[2].flag == 1
    exact = brute_force(x[:, 3])
    assert got[3].flag == 0 and len(got[3].entries) == 8 and all(set(c) <= {1, 3} and c for c, _ in got[3].entries)
    assert all(lg <= exact[tuple(c)] + 1e-12 for c, lg in got[3].entries)
    assert got[4].flag == 0 and [c for c, _ in got[4].entries] == [list(k) for k, _ in sorted(brute_force(x[:, 4]).items(),
                                                                                            key=lambda kv: -kv[1])][:8]
    assert 1 <= len(got[4].entries) <= 4                             # "", 3, 33, 333: a beam shorter than `beam`
    y = x[:, :1].clone()
    y[3] = -float("inf")                                             # a step without a finite logit
    assert read.ctc_beam_read_host(y)[0] == read.BeamDecoded([], 1)
    assert all(abs(lg - read.ctc_string_logp_host(x[:, 4], k)) <= 1e-12 for k, lg in got[4].entries)


def test_exact_ties_go_to_the_lower_key():
    """all logits equal: step 1 ties the stay candidate (key 0) with the three extensions (keys 1, 2, 3); step 2 ties the stay
    candidates of 1, 2, 3 (keys 4, 8, 12), then the empty string's (key 0) with 1+2 (key 6), 1+3 (7), 2+1 (9), ..."""
    from tatt_amd import read
    got = read.ctc_beam_read_host(torch.zeros(2, 1, 4), beam=5, nbest=5, details=True)[0]
    assert [c for c, _ in got.entries] == [[1], [2], [3], [], [1, 2]] and got.margin == 0.0
    assert got.entries[0][1] == got.entries[1][1] == got.entries[2][1] and got.entries[3][1] == got.entries[4][1]
    assert abs(got.entries[0][1] - math.log(3 / 16)) <= 1e-15 and abs(got.entries[3][1] - math.log(1 / 16)) <= 1e-15


def test_longdouble_runs_the_same_search():
    import numpy as np
    from tatt_amd import read
    x, want = beam_case(CASES[2])
    wide = read.ctc_beam_read_host(x, 8, 4, real=np.longdouble)
    for w, l in zip(want, wide):
        assert [c for c, _ in w.entries] == [c for c, _ in l.entries]
        assert max(abs(float(a[1] - b[1])) for a, b in zip(w.entries, l.entries)) <= 1e-12


def test_value_errors():
    from tatt_amd import read
    x = beam_logits(3, 1, 3, 3.0, 50)
    for kw in ({"beam": 0, "nbest": 0}, {"beam": 4, "nbest": 5}, {"beam": 4, "nbest": 0}):
        with pytest.raises(ValueError):
            read.ctc_beam_read_host(x, **kw)
    with pytest.raises(ValueError):
        read.ctc_beam_read_host(x[0])
    lim = read.beam_limits()
    assert lim == {"steps": 256, "classes": 64, "beam": 16, "nodes": 1 + 256 * 16, "table": lim["table"]}
    assert lim["table"] > 2 * lim["nodes"] and (lim["steps"], lim["classes"]) == (read.read_limits()["steps"], read.read_limits()["classes"])
    module = torch.nn.Linear(1, 1)                                   # the keywords are checked before the module is looked at
    with pytest.raises(ValueError, match="decode"):
        read.LineReader(module, decode="viterbi")
    for kw in ({"beam": 17}, {"beam": 4, "nbest": 5}, {"nbest": 0}, {"beam": 8.0}):
        with pytest.raises(ValueError, match="nbest <= beam"):
            read.LineReader(module, decode="beam", **kw)
    from tatt_amd import io
    assert io.BeamReading is read.BeamReading and io.ctc_beam_read_host is read.ctc_beam_read_host
    assert io.ctc_string_logp_host is read.ctc_string_logp_host and io.beam_limits is read.beam_limits


def test_record_round_trip():
    from tatt_amd import read
    cap, nbest = 5, 3
    es = read.beam_entry_words(cap)
    assert es == 10 and read.beam_record_words(cap, nbest) == 32 and read.beam_entry_words(6) == 10

    def entry(logp, classes):
        lo, hi = struct.unpack("<ii", struct.pack("<d", logp))
        return [lo, hi, len(classes), 0] + classes + [-1] * (es - 4 - len(classes))
    a = -0.1234567890123456789                                       # (not representable in fp32: the float64 travels as it is)
    rows = [[2, 0] + entry(a, [3, 1, 36]) + entry(-7.5, []) + [-77] * es + [-77] * 3,
            [0, 1] + [-77] * (3 * es + 3),
            [3, 0] + entry(0.0, [1, 2, 3, 4, 5]) + entry(-1e-300, [9]) + entry(-745.5, [2, 2]) + [-77] * 3]
    got = read.parse_beam_records(torch.tensor(rows, dtype=torch.int32), cap, nbest)
    assert got[0] == read.BeamDecoded([([3, 1, 36], a), ([], -7.5)], 0)
    assert got[1] == read.BeamDecoded([], 1)
    assert got[2] == read.BeamDecoded([([1, 2, 3, 4, 5], 0.0), ([9], -1e-300), ([2, 2], -745.5)], 0)
    r = read._beam_reading(got[0], 120, False)
    assert r == read.BeamReading("20z", a, [("20z", a), ("", -7.5)], 120, False)
    f = read._beam_reading(got[1], 100, True)
    assert f.text == "" and math.isnan(f.logp) and f.alternatives == [] and f.rw == 100 and f.squeezed
    with pytest.raises(ValueError):
        read.parse_beam_records(torch.tensor([[4, 0] + [0] * 30], dtype=torch.int32), cap, nbest)
