"""Reading against a format on the host (tatt_amd/read.py: Pattern, ctc_pattern_mass_host, ctc_beam_pattern_read_host), the
specifications of csrc/ctcpat.hip and of the pattern instantiation of csrc/ctcbeam.hip.  Yardsticks: `re.fullmatch` for the compiler,
brute force over all C^T alignments (in np.longdouble) for the mass and the search, the exact forward recursion and the lexicon's logz
where brute force cannot go.  This file also holds the case list of tests/test_pattern_device_gpu.py and asserts, on the CPU, that the
specification's own selection margins exceed 100 x the bar on every row of every case, so that the GPU test leaves no row out.  No GPU.

The bars.  logp: that of the plain search, 4 x |float64 - longdouble| of the specification + T x 2^-52 x max |logp|.  mass:
4 x |float64 - longdouble| of its specification + T x (S + C + 8) x 2^-52: a forward bound, not a measurement -- every quantity is a
sum of at most S + C non-negative terms, whatever its order, times a soft-max value good to a few ulps, compounded over T steps, once
for each side."""
import itertools
import math
import random
import re

import numpy as np
import pytest
import torch

from tests.test_beam import beam_logits

PLATE = r"[a-z]{2}\d{2}[a-z]{3}"
READER = "-0123456789abcdefghijklmnopqrstuvwxyz"
WIDE = READER + "!#%&',/:;<=>@_`~\"" + "äöüßéèàçñø"     # 64 classes, none of them syntax
# (T, B, C, beam, nbest, s, seed, spec, alphabet): the shapes tests/test_pattern_device_gpu.py runs on the device.  Seeds: the first for
# which every row's margin exceeds 100 x the bar and the property the case is there for holds (asserted below)
PATTERN_CASES = (
    (1, 1, 2, 1, 1, 3.0, 11, "a?", "-a"),
    (3, 2, 3, 16, 16, 3.0, 12, "a*b?a?", "-ab"),
    (26, 3, 37, 8, 4, 3.0, 13, PLATE, READER),
    (64, 17, 37, 5, 5, 3.0, 14, "[ab]{0,30}(c[ab]*)?", READER),      # three characters in play: prefixes leave the beam and come back
    (256, 2, 37, 16, 4, 3.0, 15, ".{40,63}", READER),                # 64 states, the entries end in states 40 .. 63; 256 steps
    (7, 1, 64, 16, 1, 3.0, 16, ".{2,5}", WIDE),                      # the class limit
    (26, 8, 37, 8, 4, 8.0, 17, PLATE, READER),                       # sharp logits: the plain beam's best string is no plate on any row
    (12, 6, 37, 4, 4, 8.0, 18, r"[a-z]+\d", READER),                 # rows that end without an accepting entry, their mass finite
    (66, 1, 64, 4, 2, 3.0, 19, ".{40,63}", WIDE),                    # 64 states over 64 classes: the mass kernel's 69,632 bytes of LDS
)
REENTRY, STATES64, NOT_PLAIN, NO_ENTRY = PATTERN_CASES[3], PATTERN_CASES[4], PATTERN_CASES[6], PATTERN_CASES[7]
_cache = {}


def pattern_case(case):
    """-> (logits, Pattern, the specification's result with details, the same in np.longdouble); computed once and shared, never changed"""
    if case not in _cache:
        from tatt_amd import read
        T, B, C, beam, nbest, s, seed, spec, alphabet = case
        x, pat = beam_logits(T, B, C, s, seed), read.Pattern(spec, alphabet)
        _cache[case] = (x, pat, read.ctc_beam_pattern_read_host(x, pat, beam, nbest, details=True),
                        read.ctc_beam_pattern_read_host(x, pat, beam, nbest, real=np.longdouble))
    return _cache[case]


def pattern_bars(T, S, C, want, wide):
    """-> (the bar on logp, the bar on mass, |float64 - longdouble| of logp, of mass) from the specification alone; strings must agree"""
    dist = top = dm = 0.0
    for w, l in zip(want, wide):
        assert w.flag == l.flag and [c for c, _ in w.entries] == [c for c, _ in l.entries]
        for a, b in zip(w.entries, l.entries):
            dist, top = max(dist, abs(float(np.longdouble(a[1]) - b[1]))), max(top, abs(a[1]))
        if not w.flag and math.isfinite(w.mass):
            dm = max(dm, abs(float(np.longdouble(w.mass) - l.mass)))
        else:
            assert w.flag or w.mass == float(l.mass)
    return 4 * dist + T * 2.0 ** -52 * top, 4 * dm + T * (S + C + 8) * 2.0 ** -52, dist, dm


def flagged_lines():
    """six lines of six steps over "-abc": clean | NaN | +inf | no blank, no b | a and b never | a step without a finite logit"""
    inf = float("inf")
    x = beam_logits(6, 6, 4, 3.0, 40)
    x[2, 1, 3] = float("nan")
    x[5, 2, 0] = inf
    x[:, 3, 0] = -inf
    x[:, 3, 2] = -inf
    x[:, 4, 1:3] = -inf
    x[3, 5] = -inf
    return x, "[ac]{1,3}b?"


def brute_force_wide(row):
    """row: (T, C) logits -> {string: probability as np.longdouble}: every alignment's probability from a soft-max in np.longdouble"""
    x = row.numpy().astype(np.longdouble)
    e = np.exp(x - x.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    T, C = p.shape
    mass = {}
    for path in itertools.product(range(C), repeat=T):
        string = tuple(c for i, c in enumerate(path) if c != 0 and (i == 0 or c != path[i - 1]))
        v = np.longdouble(1.0)
        for t, c in enumerate(path):
            v = v * p[t, c]
        mass[string] = mass.get(string, np.longdouble(0.0)) + v
    return mass


# ---- the compiler -----------------------------------------------------------------------------------------------------------------------
SPECS_ABC = ("abc", "a.c", "[ab]c*", "[^a]+", "[a-c]{2}", "a|bc|", "(ab)*c?", "(?:a|b){1,3}c", "a?b+c*", "(a|b)*abb", "a{0}b{2,4}",
             ".*a.{2}", "(a(b|c)?)+", "[^ab]|ab{2}", "", "()", "(a|)(b|)c{3}")
SPECS_DIGITS = (r"\d+a?", r"[\da]{2}", r"a\d{1,2}|\d", r"[^\d]*")


@pytest.mark.parametrize("spec,alphabet", [(s, "-abc") for s in SPECS_ABC] + [(s, "-a01") for s in SPECS_DIGITS])
def test_pattern_accepts_what_re_fullmatch_accepts(spec, alphabet):
    """EVERY string up to length 6 over the three characters"""
    from tatt_amd import read
    pat = read.Pattern(spec, alphabet)
    n = 0
    for length in range(7):
        for chars in itertools.product(alphabet[1:], repeat=length):
            s = "".join(chars)
            assert pat.accepts(s) == bool(re.fullmatch(spec, s)), (spec, s)
            n += 1
    assert n == 1093 and pat.table.shape == (pat.n_states, 4) and bool((pat.table[:, 0] == 255).all())
    assert pat.table.dtype == pat.accept.dtype == np.uint8 and pat.accept.shape == (pat.n_states,)
    live = pat.table[pat.table != 255]
    assert live.size == 0 or int(live.max()) < pat.n_states


@pytest.mark.parametrize("spec", (PLATE, r"\d{1,2}[./]\d{1,2}[./](19|20)\d{2}".replace("[./]", "[a-b]"), r"[a-z]{4}\d{6,7}",
                                  r"(\d{3}){1,2}(ab|cd)?[^0-9a-w]", r"[A-Z]{2}\d\d ?[A-Z]{3}".replace(" ?", "")))
def test_pattern_on_the_reader_alphabet(spec):
    """seeded samples over the full alphabet: random strings, members made from the spec's shape, and members with one character changed"""
    from tatt_amd import read
    pat, rng, chars = read.Pattern(spec), random.Random(7), READER[1:]
    low = spec.lower()                                               # (upper-case letters are lower-cased, as Lexicon does)
    members = set()
    for _ in range(4000):
        s = "".join(rng.choice(chars) for _ in range(rng.randrange(0, 14)))
        assert pat.accepts(s) == bool(re.fullmatch(low, s)), (spec, s)
        members.add(s) if pat.accepts(s) else None
    # walk the DFA at random: every string that ends in an accepting state is a member, and its mutants are judged alike
    for _ in range(300):
        q, s = 0, ""
        for _ in range(20):
            if pat.accept[q] and rng.random() < 0.3:
                break
            nxt = [c for c in range(1, 37) if pat.table[q, c] != 255]
            if not nxt:
                break
            c = rng.choice(nxt)
            q, s = int(pat.table[q, c]), s + READER[c]
        assert pat.accepts(s) == bool(re.fullmatch(low, s)), (spec, s)
        members.add(s) if pat.accepts(s) else None
        if s:
            k = rng.randrange(len(s))
            m = s[:k] + rng.choice(chars) + s[k + 1:]
            assert pat.accepts(m) == bool(re.fullmatch(low, m)), (spec, m)
            assert pat.accepts(s.upper()) == pat.accepts(s)
    assert len(members) >= 50
    assert not pat.accepts("#") and not pat.accepts("-")


def test_the_dfa_is_minimal():
    from tatt_amd import read
    assert read.Pattern(PLATE).n_states == 8 and read.Pattern(".*").n_states == 1 and read.Pattern(".{63}").n_states == 64
    assert read.Pattern("a|b|c", "-abc").n_states == 2 and read.Pattern("(a|b)*abb", "-ab").n_states == 4
    assert read.Pattern("(ab|ac)(d|d)", "-abcd").n_states == 4      # equivalent subsets are merged
    plate = read.Pattern(PLATE)
    assert plate.accept.tolist() == [0] * 7 + [1] and bool((plate.table[7] == 255).all())      # the start is 0, no dead state is kept
    assert plate.table[0, 11:].tolist() == [1] * 26 and plate.table[0, :11].tolist() == [255] * 11
    assert read.Pattern(".*").table.tolist() == [[255] + [0] * 36]
    assert read.pattern_limits() == {"steps": 256, "classes": 64, "states": 64, "beam": 16}
    assert (read.Pattern.STEPS, read.Pattern.CLASSES, read.Pattern.STATES, read.Pattern.BEAM) == (256, 64, 64, 16)
    with pytest.raises(ValueError, match="65 states"):
        read.Pattern(".{64}")
    with pytest.raises(ValueError, match="matches no string"):
        read.Pattern("[^a-z0-9]")
    with pytest.raises(ValueError, match="classes"):
        read.Pattern("a", WIDE + "$")
    wide = read.Pattern("ab", "-ab").table_for(5)
    assert wide.shape == (3, 5) and bool((wide[:, 3:] == 255).all())
    with pytest.raises(ValueError):
        read.Pattern("ab", "-ab").table_for(2)


@pytest.mark.parametrize("spec,at", (("a**", 2), ("a*?", 2), ("a*+", 2), ("a{2}{3}", 4), ("^a", 0), ("a$", 1), (r"\w", 0), (r"(a)\1", 3),
                                     (r"a\b", 1), ("(?=a)", 0), ("(?!a)", 0), ("(?<=a)b", 0), ("(?i)a", 0), ("(?P<n>a)", 0), ("a{2,}", 1),
                                     ("a{,2}", 1), ("a{257}", 1), ("a{3,2}", 1), ("a{1,257}", 1), ("[b-a]", 1), ("(a", 0), ("a)", 1),
                                     ("[]", 0), ("[a", 0), ("#", 0), ("ab#", 2), ("[a#]", 2), ("a|*", 2), ("*a", 0), ("a{x}", 1),
                                     ("a]", 1), ("a}", 1), (r"[\w]", 1), ("[a-]", 2), ("a-b", 1), (r"\D", 0)))
def test_everything_else_is_refused_with_its_position(spec, at):
    from tatt_amd import read
    with pytest.raises(ValueError, match=r"at position %d of " % at):
        read.Pattern(spec)
    with pytest.raises(ValueError):
        read.Pattern(["a"])


# ---- the mass ----------------------------------------------------------------------------------------------------------------------------
def _mass_bar(x, pat):
    from tatt_amd import read
    T, B, C = x.shape
    got, wide = read.ctc_pattern_mass_host(x, pat), read.ctc_pattern_mass_host(x, pat, real=np.longdouble)
    dm = max([abs(float(np.longdouble(g.mass) - l.mass)) for g, l in zip(got, wide) if math.isfinite(g.mass)], default=0.0)
    return got, wide, 4 * dm + T * (pat.n_states + C + 8) * 2.0 ** -52


@pytest.mark.parametrize("T,C", ((5, 4), (4, 3), (1, 2), (2, 4)))
def test_the_mass_equals_brute_force(T, C):
    from tatt_amd import read
    alphabet = "-abc"[:C]
    x = beam_logits(T, 2, C, 3.0, 50 + T)
    specs = ["a[bc]{1,2}a?", ".*", "", "a+", "(a|b)*", "a{6}", "[^a]b?"] if C == 4 else ["a*b?a?", ".*", "a{6}", "ba"] if C == 3 else ["a?", "a"]
    for spec in specs:
        pat = read.Pattern(spec, alphabet)
        got, _, bar = _mass_bar(x, pat)
        for b, g in enumerate(got):
            total = sum((v for k, v in brute_force_wide(x[:, b]).items() if re.fullmatch(spec, "".join(alphabet[c] for c in k))),
                        np.longdouble(0.0))
            assert g.flag == 0
            if total == 0:
                assert g.mass == -math.inf and spec == "a{6}"        # members exist, but no alignment of T steps spells one
            else:
                err = abs(float(np.longdouble(g.mass) - np.log(total)))
                print("T %d C %d %r line %d: mass %.17g, |mass - brute force| %.3g, bar %.3g" % (T, C, spec, b, g.mass, err, bar))
                assert err <= bar
            if spec == ".*":
                assert abs(g.mass) <= bar


def test_the_mass_of_one_word_and_of_a_word_list():
    from tatt_amd import read
    x = beam_logits(26, 3, 37, 3.0, 60)
    got, _, bar = _mass_bar(x, read.Pattern("stop"))
    word = read.Lexicon(["stop"]).classes[0]
    for b, g in enumerate(got):
        want = read.ctc_string_logp_host(x[:, b], word, real=np.longdouble)
        assert abs(float(np.longdouble(g.mass) - want)) <= bar, (b, g.mass, want, bar)
    got, _, bar = _mass_bar(x, read.Pattern("stop|yield|exit"))
    want = read.ctc_lexicon_read_host(x, read.Lexicon(["stop", "yield", "exit"]), real=np.longdouble)
    for g, w in zip(got, want):
        assert abs(float(np.longdouble(g.mass) - w.logz)) <= bar, (g.mass, w.logz, bar)
    got, _, bar = _mass_bar(x, read.Pattern(".*"))
    assert all(abs(g.mass) <= bar for g in got)
    short = read.ctc_pattern_mass_host(x[:3], read.Pattern("stop"))  # four characters in three steps
    assert all(g.mass == -math.inf and g.flag == 0 for g in short)


def test_the_mass_of_flagged_lines_and_its_arguments():
    from tatt_amd import read
    x, spec = flagged_lines()
    got = read.ctc_pattern_mass_host(x, read.Pattern(spec, "-abc"))
    assert [g.flag for g in got] == [0, 1, 1, 0, 0, 1]
    assert all(math.isnan(g.mass) == bool(g.flag) for g in got) and got[4].mass > -math.inf
    none = read.ctc_pattern_mass_host(x, read.Pattern("b", "-abc"))
    assert none[3].mass == -math.inf and none[4].mass == -math.inf and none[0].mass > -math.inf
    with pytest.raises(ValueError, match="37 classes"):
        read.ctc_pattern_mass_host(x, "a")                           # a string is compiled over the reader's alphabet
    with pytest.raises(ValueError):
        read.ctc_pattern_mass_host(x, read.Pattern("a", WIDE))       # more classes than the logits
    with pytest.raises(ValueError):
        read.ctc_pattern_mass_host(x[0], read.Pattern("a", "-abc"))
    with pytest.raises(ValueError):
        read.ctc_pattern_mass_host(x, 7)
    # an underflowing step: the rescale keeps the mass where log-space arithmetic has it
    y = torch.zeros(200, 1, 3)
    y[:, 0, 1] = 80.0
    m = read.ctc_pattern_mass_host(y, read.Pattern("", "-ab"))[0].mass            # 200 steps of e^-80: far below the smallest double
    assert abs(m - read.ctc_string_logp_host(y[:, 0], [])) <= 1e-9 * abs(m) and m < -15000


# ---- the search --------------------------------------------------------------------------------------------------------------------------
def test_an_exhaustive_pattern_beam_equals_brute_force():
    from tatt_amd import read
    case = PATTERN_CASES[1]
    T, B, C, beam, nbest, s, seed, spec, alphabet = case
    x, pat, want, wide = pattern_case(case)
    plain = read.ctc_beam_read_host(x, beam, nbest)
    every = read.ctc_beam_pattern_read_host(x, read.Pattern(".*", alphabet), beam, nbest)
    bar, mbar, _, _ = pattern_bars(T, pat.n_states, C, want, wide)
    for b, w in enumerate(want):
        exact = brute_force_wide(x[:, b])
        assert len(plain[b].entries) == len(exact)                   # the beam holds every string there is
        assert every[b].entries == plain[b].entries                  # .* is the plain search, bit for bit
        kept = sorted(((k, v) for k, v in exact.items() if re.fullmatch(spec, "".join(alphabet[c] for c in k))), key=lambda kv: -kv[1])
        assert 0 < len(kept) < len(exact)
        assert [tuple(c) for c, _ in w.entries] == [k for k, _ in kept]
        assert max(abs(float(np.longdouble(lg) - np.log(v))) for (_, lg), (_, v) in zip(w.entries, kept)) <= bar + 1e-15
        total = sum((v for _, v in kept), np.longdouble(0.0))
        assert abs(float(np.longdouble(w.mass) - np.log(total))) <= mbar
        lse = math.log(sum(math.exp(lg) for _, lg in w.entries))     # an exhaustive beam's entries add up to the mass
        assert abs(lse - w.mass) <= mbar + 16 * 2.0 ** -52


def test_dot_star_is_the_plain_search():
    from tatt_amd import read
    for case in (PATTERN_CASES[2], PATTERN_CASES[7]):
        T, B, C, beam, nbest, s, seed, spec, alphabet = case
        x = beam_logits(T, B, C, s, seed)
        plain = read.ctc_beam_read_host(x, beam, nbest, details=True)
        got = read.ctc_beam_pattern_read_host(x, ".*", beam, nbest, details=True)
        for g, p in zip(got, plain):
            assert g.entries == p.entries and (g.flag, g.margin, g.reentry) == (p.flag, p.margin, p.reentry)
    with pytest.raises(ValueError):
        read.ctc_beam_pattern_read_host(x, ".*", 4, 5)
    with pytest.raises(ValueError):
        read.ctc_beam_pattern_read_host(x, None)
    fx, spec = flagged_lines()
    got = read.ctc_beam_pattern_read_host(fx, read.Pattern(spec, "-abc"), 8, 8, details=True)
    assert [g.flag for g in got] == [0, 1, 1, 0, 0, 1] and all(g.entries == [] and math.isnan(g.mass) for g in got if g.flag)
    assert all(g.entries for g in got if not g.flag)


@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda c: "T%d-B%d-C%d-beam%d-nbest%d-s%g" % c[:6])
def test_the_gpu_cases_leave_no_row_out(case):
    """every entry is accepted, every logp <= mass + bar, and on EVERY row the specification's neighbour margins exceed 100 x the bar"""
    from tatt_amd import read
    T, B, C, beam, nbest, s, seed, spec, alphabet = case
    x, pat, want, wide = pattern_case(case)
    bar, mbar, dist, dm = pattern_bars(T, pat.n_states, C, want, wide)
    print("case %s %r: S %d, bar %.3g (float64 - longdouble %.3g), mass bar %.3g (%.3g), smallest margin %.3g, entries %s, re-entries %d"
          % (case[:6], spec, pat.n_states, bar, dist, mbar, dm, min(w.margin for w in want), [len(w.entries) for w in want],
             sum(w.reentry for w in want)))
    for b, w in enumerate(want):
        assert w.flag == 0 and w.margin > 100 * bar, (b, w.margin, bar)
        assert math.isfinite(w.mass)
        for classes, logp in w.entries:
            assert pat.accepts("".join(alphabet[c] for c in classes)) and logp <= w.mass + bar + mbar
            assert abs(read.ctc_string_logp_host(x[:, b], classes) - logp) <= 1e-9 or logp < read.ctc_string_logp_host(x[:, b], classes)
    plain = read.ctc_beam_read_host(x, beam, nbest)
    if case == REENTRY:
        assert sum(w.reentry for w in want) >= 1
    if case == STATES64:
        assert pat.n_states == 64 and all(len(c) >= 40 for w in want for c, _ in w.entries) and all(w.entries for w in want)
    if case == NOT_PLAIN:
        assert all(w.entries for w in want)
        assert not any(pat.accepts("".join(alphabet[c] for c in p.entries[0][0])) for p in plain)
    if case == NO_ENTRY:
        assert any(not w.entries for w in want) and any(w.entries for w in want)
    if case[0] == 7:
        assert pat.n_classes == 64 and any(c >= 37 for w in want for cl, _ in w.entries for c in cl)


def test_reader_arguments_are_checked_before_any_device_work():
    """the ValueErrors of `LineReader(pattern=...)` that need no device: raised before the CRNN is looked at"""
    from tatt_amd import read
    with pytest.raises(ValueError, match="pattern= goes with decode='beam'"):
        read.LineReader(None, decode="greedy", pattern="a")
    with pytest.raises(ValueError, match="pattern= goes with decode='beam'"):
        read.LineReader(None, decode="lexicon", lexicon=["a"], pattern="a")
    lm = read.CharLM(np.log(np.full((37,), 1.0 / 37)))
    with pytest.raises(ValueError, match="do not go together"):
        read.LineReader(None, decode="beam", lm=lm, pattern="a")
    with pytest.raises(ValueError, match="at position 0"):
        read.LineReader(None, decode="beam", pattern="^a")
    with pytest.raises(ValueError, match="states"):
        read.LineReader(None, decode="beam", pattern=".{64}")
    with pytest.raises(ValueError, match="states the classes it emits"):
        read.LineReader(None, decode="beam", pattern="a")            # the one upload is made for the classes of the logits
    assert read.pattern_record_words(26, 4) == read.beam_record_words(26, 4) + 4
    row = torch.tensor([[0, -1074790400, 0, 0], [0, 2146959360, 1, 0]], dtype=torch.int32)      # -1.0 | NaN, flagged
    got = read.parse_pattern_mass(row)
    assert got[0] == read.PatternMass(-1.0, 0) and math.isnan(got[1].mass) and got[1].flag == 1
