"""CTC forced alignment on the host: `read.ctc_align_host` (the specification of csrc/ctcalign.hip) against brute force over all C^T
alignments with `==`, its stated tie order, -inf columns, empty and infeasible strings, the record layout (`pack_strings`,
`parse_align_records`) and the refusals.  The cases of the device test and of tools/align_host_check.py are built here."""
import itertools
import math
import random
import struct

import pytest
import torch

from tests.test_words import log_softmax_rows

NEG = -math.inf
BITS = lambda v: struct.pack("<d", v)
FILL = -77


# ---- brute force ----------------------------------------------------------------------------------------------------------------------
def collapse(path):
    out, last = [], 0
    for c in path:
        if c != 0 and c != last:
            out.append(c)
        last = c
    return tuple(out)


def brute_force(lp):
    """-> {collapsed string: the largest left-to-right path sum over its alignments} over all C^T alignments"""
    T, C = len(lp), len(lp[0])
    best = {}
    for path in itertools.product(range(C), repeat=T):
        v = lp[0][path[0]]
        for t in range(1, T):
            v = v + lp[t][path[t]]
        key = collapse(path)
        if v > best.get(key, NEG):
            best[key] = v
    return best


def random_lp(T, C, seed, holes=False):
    """float64 log-soft-max rows of seeded fp32 logits; with `holes` some logits are -inf (never a whole step)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, 1, C, generator=g) * 3.0
    if holes:
        mask = torch.rand(T, 1, C, generator=g) < 0.25
        mask[:, :, seed % C] = False
        x = x.masked_fill(mask, NEG)
    return log_softmax_rows(x, 0)


def check_alignment(lp, classes, al):
    """what every result must satisfy on its own: ordered, disjoint spans, blanks elsewhere, and the path's sum IS logp"""
    T, L = len(lp), len(classes)
    assert al.flag == 0
    if al.logp == NEG:
        assert al.spans == [] and al.char_logp == []
        return None
    assert len(al.spans) == len(al.char_logp) == L
    path, end = [0] * T, -1
    for k, ((f, l), c) in enumerate(zip(al.spans, classes)):
        assert 0 <= f <= l < T and f > end, (k, al.spans)
        if k >= 1 and classes[k - 1] == c:
            assert f > end + 1, (k, al.spans)                        # a blank between equal neighbours
        for t in range(f, l + 1):
            path[t] = c
        end = l
        acc = lp[f][c]
        for t in range(f + 1, l + 1):
            acc = acc + lp[t][c]
        assert BITS(acc) == BITS(al.char_logp[k]), (k, acc, al.char_logp[k])
    assert collapse(path) == tuple(classes)
    v = lp[0][path[0]]
    for t in range(1, T):
        v = v + lp[t][path[t]]
    assert BITS(v) == BITS(al.logp), (v, al.logp, path)
    return path


def strings_of(best, L, rng, C):
    """strings of length L to try: one seen among the alignments (feasible), one drawn freely (repeats and infeasible ones included)"""
    seen = sorted(k for k in best if len(k) == L)
    out = [list(rng.choice(seen))] if seen else []
    out.append([rng.randrange(1, C) for _ in range(L)])
    return out


def test_the_specification_equals_brute_force():
    from tatt_amd import read
    n = infeasible = repeats = 0
    for T, C in ((1, 2), (1, 3), (2, 2), (2, 3), (3, 2), (3, 3), (3, 4), (4, 2), (4, 3), (5, 2), (5, 3), (5, 4), (6, 2), (6, 3), (7, 2),
                 (7, 3)):
        for seed in range(3):
            lp = random_lp(T, C, 100 * T + 10 * C + seed, holes=seed == 2)
            best = brute_force(lp)
            rng = random.Random(seed + 7 * T)
            for L in range(T + 1):
                for classes in strings_of(best, L, rng, C):
                    al = read.ctc_align_host(lp, classes)
                    want = best.get(tuple(classes), NEG)
                    assert al.logp == want and (want == NEG or BITS(al.logp) == BITS(want)), (T, C, seed, classes, al.logp, want)
                    check_alignment(lp, classes, al)
                    n += 1
                    infeasible += want == NEG
                    repeats += any(a == b for a, b in zip(classes, classes[1:]))
    print("%d cases against brute force, %d infeasible, %d with equal neighbours" % (n, infeasible, repeats))
    assert n >= 324 and infeasible >= 10 and repeats >= 10


def test_the_stated_tie_order_on_all_equal_logits():
    """every comparison a tie: a state stays; the end is state 2 L -- so the characters come as early as they can"""
    from tatt_amd import read
    for T, C in ((5, 3), (9, 4)):
        lp = log_softmax_rows(torch.zeros(T, 1, C), 0)
        for classes, spans in (([], []), ([1], [(0, 0)]), ([1, 2], [(0, 0), (1, 1)]), ([1, 1], [(0, 0), (2, 2)]),
                               ([2, 1, 2], [(0, 0), (1, 1), (2, 2)]), ([1, 1, 2], [(0, 0), (2, 2), (3, 3)])):
            al = read.ctc_align_host(lp, classes)
            assert al.spans == spans, (T, classes, al)
            check_alignment(lp, classes, al)
    lp = log_softmax_rows(torch.zeros(3, 1, 3), 0)
    assert read.ctc_align_host(lp, [1, 2, 1]).spans == [(0, 0), (1, 1), (2, 2)]          # T = L: ends in state 2 L - 1
    assert read.ctc_align_host(lp, [1, 1]).spans == [(0, 0), (2, 2)]                     # fits exactly
    assert read.ctc_align_host(lp, [1, 1, 1]) == read.Aligned([], [], NEG, 0)            # no room for the blanks
    assert read.ctc_align_host(lp, [1, 2, 1, 2]) == read.Aligned([], [], NEG, 0)         # T too short


def test_minus_infinity_columns_and_the_empty_string():
    from tatt_amd import read
    x = torch.zeros(4, 1, 3)
    x[:, 0, 2] = NEG                                                 # class 2 never
    lp = log_softmax_rows(x, 0)
    assert read.ctc_align_host(lp, [2]) == read.Aligned([], [], NEG, 0)
    assert read.ctc_align_host(lp, [1, 2]) == read.Aligned([], [], NEG, 0)
    check_alignment(lp, [1], read.ctc_align_host(lp, [1]))
    x = torch.zeros(4, 1, 3)
    x[1:, 0, 0] = NEG                                                # no blank after step 0: "1" must hold to the end
    lp = log_softmax_rows(x, 0)
    assert read.ctc_align_host(lp, [1]).spans == [(0, 3)]
    assert read.ctc_align_host(lp, []) == read.Aligned([], [], NEG, 0)
    assert read.ctc_align_host(lp, [1, 2]).spans == [(0, 0), (1, 3)]
    lp = random_lp(6, 3, 5)
    al = read.ctc_align_host(lp, [])                                 # L = 0: the all-blank path
    v = lp[0][0]
    for t in range(1, 6):
        v = v + lp[t][0]
    assert al == read.Aligned([], [], v, 0)


def test_reading_from_logits_flags_what_the_other_decoders_flag():
    from tatt_amd import read
    x = torch.randn(5, 4, 4, generator=torch.Generator().manual_seed(3))
    x[2, 1, 3] = math.nan
    x[0, 2, 1] = math.inf
    x[4, 3, :] = NEG
    out = read.ctc_align_read_host(x, [[1, 2], [1], [2], [3]])
    assert out[0].flag == 0 and out[0] == read.ctc_align_host(log_softmax_rows(x, 0), [1, 2])
    for al in out[1:]:
        assert al.flag == 1 and al.spans == [] and al.char_logp == [] and math.isnan(al.logp)
    with pytest.raises(ValueError):
        read.ctc_align_read_host(x, [[1]])


def write_record(al, cap_len, extra=0):
    """an Aligned as the row tatt_ctc_align writes, over a row of FILL"""
    row = [FILL] * (4 + 4 * cap_len + extra)
    row[0], row[1] = len(al.spans), al.flag
    row[2:4] = struct.unpack("<ii", BITS(al.logp))
    for k, (f, l) in enumerate(al.spans):
        row[4 + 2 * k:6 + 2 * k] = [f, l]
        row[4 + 2 * cap_len + 2 * k:6 + 2 * cap_len + 2 * k] = struct.unpack("<ii", BITS(al.char_logp[k]))
    return row


def test_pack_strings_and_the_record_round_trip():
    import numpy as np
    from tatt_amd import read
    assert read.align_record_words(0) == 4 and read.align_record_words(127) == 512
    table = read.pack_strings([[3, 4, 5], [], [36]], 4)
    assert table.dtype == np.int32 and table.tolist() == [[3, 0, 3, 4, 5, -1], [0, 0, -1, -1, -1, -1], [1, 0, 36, -1, -1, -1]]
    assert read.pack_strings([], 0).shape == (0, 2)
    lp = random_lp(9, 5, 1)
    als = [read.ctc_align_host(lp, [1, 2, 2]), read.ctc_align_host(lp, []), read.Aligned([], [], NEG, 0),
           read.Aligned([], [], math.nan, 1), read.Aligned([], [], math.nan, 2)]
    rec = torch.tensor([write_record(al, 6) for al in als], dtype=torch.int32)
    back = read.parse_align_records(rec, 6)
    for al, got in zip(als, back):
        assert got.spans == al.spans and got.flag == al.flag and BITS(got.logp) == BITS(al.logp)
        assert [BITS(v) for v in got.char_logp] == [BITS(v) for v in al.char_logp]
    assert read.parse_align_records(rec.numpy(), 6)[0].spans == als[0].spans
    loc = read._location(als[0], [1, 2, 2], "-abcd", 100, False, 128)
    assert loc.text == "abb" and loc.flag == 0 and loc.logp == als[0].logp and (loc.rw, loc.squeezed) == (100, False)
    assert [(c.char, c.cls, c.first, c.last, c.logp) for c in loc.chars] == [
        (ch, k, f, l, v) for ch, k, (f, l), v in zip("abb", [1, 2, 2], als[0].spans, als[0].char_logp)]
    assert [(c.x0, c.x1) for c in loc.chars] == [read.word_span_pixels(f, l, 128, 100) for f, l in als[0].spans]


def test_refusals():
    from tatt_amd import read
    assert read.align_limits() == {"steps": read.ALIGN_STEPS, "classes": read.ALIGN_CLASSES, "length": read.ALIGN_LENGTH}
    assert read.align_limits() == {"steps": 256, "classes": 64, "length": 127}
    lp = random_lp(4, 3, 2)
    for classes in ([0], [3], [1, -1], [1.0]):
        with pytest.raises(ValueError):
            read.ctc_align_host(lp, classes)
    with pytest.raises(ValueError):
        read.ctc_align_host([], [])
    with pytest.raises(ValueError, match="line 1"):
        read.pack_strings([[1], [1, 2, 3]], 2)
    for cap_len in (-1, 128, 2.0):
        with pytest.raises(ValueError):
            read.pack_strings([[1]], cap_len)
    good = write_record(read.Aligned([(0, 1)], [-0.5], -1.0, 0), 2)
    for at, v in ((0, 3), (0, -1), (1, 3), (1, -1)):
        bad = list(good)
        bad[at] = v
        with pytest.raises(ValueError):
            read.parse_align_records(torch.tensor([bad], dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        read.parse_align_records(torch.tensor([good[:-1]], dtype=torch.int32), 2)
    for decode in ("lexicon", "lexicons", "words"):
        with pytest.raises(ValueError, match="locate"):
            read.LineReader(None, decode=decode, lexicon=["a"] if decode != "lexicons" else None, locate=True)


# ---- the cases of the device test and of the host check ---------------------------------------------------------------------------
def _distinct(rng, L, C):
    """L classes in 1 .. C - 1, no equal neighbours"""
    out = []
    for _ in range(L):
        c = rng.randrange(1, C)
        while out and c == out[-1]:
            c = rng.randrange(1, C)
        out.append(c)
    return out


def device_cases():
    """-> {name: (logits (T, B, C) fp32, [one list of classes per line])}: the shapes of the issue"""
    g = lambda seed: torch.Generator().manual_seed(seed)
    rng = random.Random(41)
    out = {}
    out["one-step"] = (torch.randn(1, 2, 2, generator=g(1)), [[], [1]])
    every = [list(s) for L in range(4) for s in itertools.product((1, 2), repeat=L)]            # 15 strings; [1, 1]: fits; [1, 1, 1]: not
    x = torch.randn(3, 8, 3, generator=g(2)) * 2.0
    out["all-15-first"] = (x, every[:8])
    out["all-15-rest"] = (x, every[8:] + [[2, 1]])
    out["reader-T"] = (torch.randn(26, 3, 37, generator=g(3)) * 3.0, [[], _distinct(rng, 7, 37), _distinct(rng, 26, 37)])
    lengths = [31, 32, 33, 0, 1, 5, 12, 20, 29, 30, 34, 40, 45, 63, 64, 2, 17]
    strings = [_distinct(rng, L, 37) if i % 2 == 0 else [rng.randrange(1, 37) for _ in range(L)] for i, L in enumerate(lengths)]
    out["wave-edge"] = (torch.randn(64, 17, 37, generator=g(4)) * 3.0, strings)
    at_limit = _distinct(rng, 127, 64)
    at_limit[40] = at_limit[39]                                      # one repeat: needs its blank
    out["limit"] = (torch.randn(256, 2, 64, generator=g(5)) * 3.0, [_distinct(rng, 127, 64), at_limit])
    out["ties"] = (torch.zeros(9, 4, 5), [[], [1, 2, 3], [1, 1, 2], [4, 3, 4, 3, 4, 3, 4, 3]])
    return out


def degenerate_lines():
    """-> (logits (6, 6, 4), strings, flags): a NaN line, a +inf line and a step without a finite logit beside clean ones"""
    x = torch.randn(6, 6, 4, generator=torch.Generator().manual_seed(9))
    x[3, 1, 2] = math.nan
    x[0, 3, 0] = math.inf
    x[5, 4, :] = NEG
    x[2, 5, 1] = NEG                                                 # (a -inf logit alone is legal)
    return x, [[1, 2], [1], [3, 1], [2], [1], [1, 3]], [0, 1, 0, 1, 1, 0]


# ---- the two-stage yardstick of a launch (tests/test_align_device_gpu.py and tools/align_host_check.py) ---------------------------
LP_FILL = 12345.0


def stage_a(x, lp, index, n_rows, what):
    """(a): lp_out (B, T, C), a float64 tensor, against the specification's log-soft-max of the logits x (T, B, C) -> (bar, the
    specification's own |float64 - longdouble|, the largest |device - specification|).  The bar is measured from the specification
    alone: 4 x that distance + 2^-52 max |lp|.  A flagged line is all NaN, a line without a record row keeps the caller's fill."""
    import numpy as np
    dist = top = worst = 0.0
    clean = {}
    for b in range(x.shape[1]):
        if not 0 <= index[b] < n_rows:
            assert bool((lp[b] == LP_FILL).all()), (what, b)
            continue
        want = log_softmax_rows(x, b)
        if any(r is None for r in want):
            assert bool(torch.isnan(lp[b]).all()), (what, b)
            continue
        clean[b] = want
        for r, w in zip(want, log_softmax_rows(x, b, np.longdouble)):
            for v, u in zip(r, w):
                if v != NEG:
                    dist, top = max(dist, abs(float(np.longdouble(v) - u))), max(top, abs(v))
    bar = 4 * dist + 2.0 ** -52 * top
    for b, want in clean.items():
        for t, (r, g) in enumerate(zip(want, lp[b].tolist())):
            for c, (v, u) in enumerate(zip(r, g)):
                if v == NEG:
                    assert u == NEG, (what, b, t, c, u)
                else:
                    assert abs(u - v) <= bar, (what, b, t, c, u, v, bar)
                    worst = max(worst, abs(u - v))
    return bar, dist, worst


def expected_alignment(lp_b, length, classes, gate, C, cap_len):
    """what the device must make of a source row (stated length, the classes behind it, the gate word) on ITS OWN lp_out"""
    from tatt_amd import read
    if bool(torch.isnan(lp_b).any()) or gate < 1:
        return read.Aligned([], [], math.nan, 1)
    if not 0 <= length <= min(cap_len, 127) or any(not 1 <= c < C for c in classes[:length]):
        return read.Aligned([], [], math.nan, 2)
    return read.ctc_align_host(lp_b.tolist(), list(classes[:length]))


def stage_b(lp, sources, index, before, after, rec_at, cap_len, C, what):
    """(b): every row of the record `after` equals `before` with -- for the lines that have a row -- the alignment part replaced by the
    specification run on the device's own lp_out, BIT FOR BIT: n, flag, the 64 bits of logp, every (first, last), the 64 bits of
    every char_logp; every other word (the canary, the decode part, untouched rows) as it was.  sources[b] = (length, classes, gate).
    -> the Aligned per line (None without a row)."""
    from tatt_amd import read
    n_rows, out = before.shape[0], []
    want = [list(r) for r in before.tolist()]
    for b, (length, classes, gate) in enumerate(sources):
        r = index[b]
        if not 0 <= r < n_rows:
            out.append(None)
            continue
        al = expected_alignment(lp[b], length, classes, gate, C, cap_len)
        part = write_record(al, cap_len)
        n = len(al.spans)
        for i in list(range(4 + 2 * n)) + list(range(4 + 2 * cap_len, 4 + 2 * cap_len + 2 * n)):       # the words the device states
            want[r][rec_at + i] = part[i]
        out.append(al)
    got = after.tolist()
    for r in range(n_rows):
        w, g = want[r], got[r]
        lines = [b for b in range(len(sources)) if index[b] == r]
        if lines and out[lines[-1]].flag != 0:                       # a NaN is a NaN whatever its payload
            assert math.isnan(struct.unpack("<d", struct.pack("<ii", *g[rec_at + 2:rec_at + 4]))[0]), (what, r)
            w[rec_at + 2:rec_at + 4] = g[rec_at + 2:rec_at + 4]
        assert g == w, (what, r, [(i, a, e) for i, (a, e) in enumerate(zip(g, w)) if a != e][:8])
    return out


# ---- the launches both of them make -----------------------------------------------------------------------------------------------------
def make_launch(name, x, sources, index=None, n_rows=None, rec_at=0, cap_len=None, in_record=False, extra=6):
    """One tatt_ctc_align launch as data.  sources[b] = (stated length, classes, gate word) of line b.  in_record=False: the strings lie
    in a table of `pack_strings` layout (len_at 0, cls_at 2, no gate; row index[b]); True: in the record itself, laid out as a beam row
    ([0] the gate, [1] 0, [2:4] a logp, [4] the length, [5] 0, then the classes) with the alignment part behind it.
    -> dict(name, x, sources, index, before (the record before the launch), table (or None), len_at, cls_at, gate_at, rec_at, cap_len)"""
    T, B, C = x.shape
    index = list(range(B)) if index is None else list(index)
    n_rows = B if n_rows is None else n_rows
    width = max([len(s[1]) for s in sources] + [1])
    cap_len = min(width, 127) if cap_len is None else cap_len
    if in_record:
        len_at, cls_at, gate_at = 4, 6, 0
        rec_at = 6 + width + (width & 1)
    else:
        len_at, cls_at, gate_at = 0, 2, -1
    before = torch.full((n_rows, rec_at + 4 + 4 * cap_len + extra), FILL, dtype=torch.int32)
    table = None if in_record else torch.full((n_rows, 2 + max(width, cap_len)), -1, dtype=torch.int32)
    for b, (length, classes, gate) in enumerate(sources):
        if 0 <= index[b] < n_rows:
            row = before[index[b]] if in_record else table[index[b]]
            if in_record:
                row[0], row[1], row[5] = gate, 0, 0
            else:
                row[1] = 0
            row[len_at] = length
            row[cls_at:cls_at + len(classes)] = torch.tensor(classes, dtype=torch.int32)
    return dict(name=name, x=x, sources=sources, index=index, before=before, table=table, len_at=len_at, cls_at=cls_at, gate_at=gate_at,
                rec_at=rec_at, cap_len=cap_len)


def strided(x):
    """the same logits as a view with strides of its own (every second element of a (B, T, 2 C) buffer), offset 0"""
    T, B, C = x.shape
    buf = torch.full((B, T, 2 * C), 7.0)
    v = buf[:, :, ::2].permute(1, 0, 2)
    v.copy_(x)
    return v


def launches(lines_at_the_limit=2):
    cases = device_cases()
    plain = lambda strings: [(len(s), s, 1) for s in strings]
    out = []
    for name, (x, strings) in cases.items():
        if name == "limit":
            x, strings = x[:, :lines_at_the_limit].contiguous(), strings[:lines_at_the_limit]
        out.append(make_launch(name, x, plain(strings)))
    for name in ("reader-T", "wave-edge"):
        x, strings = cases[name]
        out.append(make_launch(name + "-strided", strided(x), plain(strings)))
    # strings the DEVICE refuses (flag 2) beside good ones: a stated length of 128 and of -1, the classes 0 and C
    x = torch.randn(12, 6, 5, generator=torch.Generator().manual_seed(6))
    out.append(make_launch("refused", x, [(3, [1, 2, 3], 1), (128, [1] * 127, 1), (-1, [1], 1), (2, [1, 0], 1), (2, [5, 1], 1), (1, [4], 1)],
                           cap_len=127))
    out.append(make_launch("over-cap", x, [(3, [1, 2, 3], 1), (4, [1, 2, 3, 4], 1), (0, [], 1), (3, [4, 4, 1], 1), (3, [1, 2, 1], 1),
                                           (2, [2, 2], 1)], cap_len=3))
    # degenerate lines beside clean ones, the strings in the record behind a gate: flag 1 for a NaN, a +inf, a dead step and a closed gate
    x, strings, flags = degenerate_lines()
    gates = [1, 1, 0, 1, 1, 4]
    out.append(make_launch("degenerate", x, [(len(s), s, g) for s, g in zip(strings, gates)], in_record=True))
    # scattered rows in a larger record, two lines sent nowhere, the alignment part at word 2
    B, n_rows = x.shape[1], x.shape[1] + 3
    order = [n_rows - 1 - b for b in range(B)]
    order[1], order[4] = -1, n_rows
    out.append(make_launch("scattered", x, plain(strings), index=order, n_rows=n_rows, rec_at=2))
    return out


def test_the_launch_descriptions_cover_what_they_name():
    ls = {l["name"]: l for l in launches()}
    assert [len(s[1]) for s in ls["wave-edge"]["sources"]][:3] == [31, 32, 33] and ls["limit"]["cap_len"] == 127
    assert ls["all-15-first"]["sources"][:2] == [(0, [], 1), (1, [1], 1)] and (2, [1, 1], 1) in ls["all-15-first"]["sources"]
    assert (3, [1, 1, 1], 1) in ls["all-15-first"]["sources"] and (3, [2, 2, 2], 1) in ls["all-15-rest"]["sources"]
    assert not ls["reader-T-strided"]["x"].is_contiguous() and ls["degenerate"]["gate_at"] == 0 and ls["degenerate"]["rec_at"] % 2 == 0
    assert all(l["before"].shape[1] % 2 == 0 for l in ls.values())
