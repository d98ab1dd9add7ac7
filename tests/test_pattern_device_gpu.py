"""Reading against a format on the GPU (csrc/ctcbeam.hip's pattern instantiation and csrc/ctcpat.hip; read.ctc_beam_pattern_read,
read.ctc_pattern_mass, read.LineReader(decode="beam", pattern=...), infer.SuperResolver(read_pattern=...)).  Yardsticks: the host
specifications read.ctc_beam_pattern_read_host and read.ctc_pattern_mass_host in float64, themselves held to `re.fullmatch` and brute
force by tests/test_pattern.py, which also holds the case list and asserts that on EVERY row of every case the specification's selection
margin exceeds 100 x the bar: no row is left out here.  Strings, lengths and order are exact.  logp is held to the bar of the plain search,
4 x |float64 - longdouble| of the specification + T x 2^-52 x max |logp|; mass to 4 x |float64 - longdouble| of its specification +
T x (S + C + 8) x 2^-52, a forward bound (tests/test_pattern.py states it)."""
import math
import re

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests.test_beam import CASES as BEAM_CASES
from tests.test_beam import beam_case
from tests.test_lines_device_gpu import LR, _generator, _img, _same
from tests.test_pattern import PATTERN_CASES, PLATE, READER, WIDE, brute_force_wide, flagged_lines, pattern_bars, pattern_case
from tests.test_read_device_gpu import _upload

pytestmark = pytest.mark.gpu
FILL = -77


def _run(dev, x, pat, beam, nbest, cap=None):
    """one launch of each kernel on contiguous logits, rows in input order -> (BeamDecoded per line, PatternMass per line, the record
    and the mass rows on the host)"""
    from tatt_amd import read
    T, B, C = x.shape
    cap = T if cap is None else cap
    rec = torch.full((B, read.beam_record_words(cap, nbest)), FILL, dtype=torch.int32, device=dev)
    out = torch.full((B, read.PATTERN_MASS_WORDS + 3), FILL, dtype=torch.int32, device=dev)
    xd, idx = x.to(dev), torch.arange(B, dtype=torch.int32).to(dev)
    read.ctc_beam_pattern_read(xd, pat, idx, rec, cap, beam, nbest)
    read.ctc_pattern_mass(xd, pat, idx, out)
    host, mass = rec.cpu(), out.cpu()
    return read.parse_beam_records(host, cap, nbest), read.parse_pattern_mass(mass), host, mass


def _mass_err(got, want):
    if want.flag or got.flag:
        return 0.0 if got.flag == want.flag and math.isnan(got.mass) else math.inf
    return 0.0 if got.mass == want.mass else abs(got.mass - want.mass)   # (-inf equals -inf)


@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda c: "T%d-B%d-C%d-beam%d-nbest%d-s%g" % c[:6])
def test_pattern_kernels_equal_the_specifications(dev, case):
    """Measured on an MI355X: see the README, section "Reading against a format" (the bars and the distances of every case)."""
    from tatt_amd import read
    T, B, C, beam, nbest, s, seed, spec, alphabet = case
    x, pat, want, wide = pattern_case(case)
    bar, mbar, dist, dm = pattern_bars(T, pat.n_states, C, want, wide)
    got, masses, host, mass = _run(dev, x, pat, beam, nbest)
    worst = worst_m = 0.0
    for b, (g, m, w) in enumerate(zip(got, masses, want)):
        assert w.margin > 100 * bar, (b, w.margin, bar)              # (tests/test_pattern.py holds every row to this: none is left out)
        assert g.flag == m.flag == w.flag == 0 and [c for c, _ in g.entries] == [c for c, _ in w.entries], (b, g.entries, w.entries)
        worst = max([worst] + [abs(a[1] - c[1]) for a, c in zip(g.entries, w.entries)])
        worst_m = max(worst_m, _mass_err(m, w))
    print("case %s %r: S %d; logp bar %.3g (float64 - longdouble of the specification %.3g), device - specification %.3g; mass bar %.3g "
          "(%.3g), device - specification %.3g; smallest margin %.3g, entries %s, rows with a re-entry %d"
          % (case[:6], spec, pat.n_states, bar, dist, worst, mbar, dm, worst_m, min(w.margin for w in want),
             [len(w.entries) for w in want], sum(w.reentry for w in want)))
    assert worst <= bar, (worst, bar)
    assert worst_m <= mbar, (worst_m, mbar)
    es = read.beam_entry_words(T)
    for b, g in enumerate(got):                                      # the rows as the header states them
        assert host[b, 0] == len(g.entries) and host[b, 1] == 0
        for i, (c, _) in enumerate(g.entries):
            e = host[b, 2 + i * es:2 + (i + 1) * es]
            assert e[2] == len(c) and e[3] == 0 and bool((e[4 + len(c):] == -1).all())
        assert bool((host[b, 2 + len(g.entries) * es:] == FILL).all())       # entries that do not exist are not written
        assert mass[b, 2] == 0 and mass[b, 3] == 0 and bool((mass[b, read.PATTERN_MASS_WORDS:] == FILL).all())
    if beam >= 16 and C ** T <= 81:                                  # the exhaustive shape: every accepted string, as brute force orders them
        for b, (g, m) in enumerate(zip(got, masses)):
            exact = brute_force_wide(x[:, b])
            kept = sorted(((k, v) for k, v in exact.items() if re.fullmatch(spec, "".join(alphabet[c] for c in k))), key=lambda kv: -kv[1])
            assert [tuple(c) for c, _ in g.entries] == [k for k, _ in kept]
            assert max(abs(float(np.longdouble(a[1]) - np.log(v))) for a, (_, v) in zip(g.entries, kept)) <= 1e-14 + bar
            assert abs(float(np.longdouble(m.mass) - np.log(sum((v for _, v in kept), np.longdouble(0.0))))) <= mbar


@pytest.mark.parametrize("case", (BEAM_CASES[2], BEAM_CASES[7], BEAM_CASES[5]), ids=lambda c: "T%d-B%d-C%d-beam%d" % c[:4])
def test_dot_star_is_the_plain_kernel_bit_for_bit(dev, case):
    """`.*` constrains nothing: the words of tatt_ctc_beam_read, every one of them (BEAM_CASES[7]: prefixes re-enter the beam)"""
    from tatt_amd import read
    T, B, C, beam, nbest, s, seed = case
    x, _ = beam_case(case)
    pat = read.Pattern(".*", WIDE[:C])
    assert pat.n_states == 1
    got, masses, host, _ = _run(dev, x, pat, beam, nbest)
    plain = torch.full_like(host, FILL).to(dev)
    read.ctc_beam_read(x.to(dev), torch.arange(B, dtype=torch.int32).to(dev), plain, T, beam, nbest)
    assert torch.equal(host, plain.cpu())
    assert all(m.flag == 0 and abs(m.mass) <= T * (1 + C + 8) * 2.0 ** -52 for m in masses)     # every string is a member: log 1


def test_flagged_lines_beside_clean_ones(dev):
    from tatt_amd import read
    x, spec = flagged_lines()
    pat = read.Pattern(spec, "-abc")
    want = read.ctc_beam_pattern_read_host(x, pat, 8, 8, details=True)
    wide = read.ctc_beam_pattern_read_host(x, pat, 8, 8, real=np.longdouble)
    assert [w.flag for w in want] == [0, 1, 1, 0, 0, 1]
    bar, mbar, _, _ = pattern_bars(6, pat.n_states, 4, want, wide)
    got, masses, host, mass = _run(dev, x, pat, 8, 8)
    for b, (g, m, w) in enumerate(zip(got, masses, want)):
        assert g.flag == m.flag == w.flag and [c for c, _ in g.entries] == [c for c, _ in w.entries], (b, g, w)
        assert all(abs(a[1] - c[1]) <= bar for a, c in zip(g.entries, w.entries)) and _mass_err(m, w) <= mbar
        if w.flag:
            assert host[b, 0] == 0 and host[b, 1] == 1 and bool((host[b, 2:] == FILL).all())
            assert math.isnan(m.mass) and mass[b, 2] == 1 and bool((mass[b, read.PATTERN_MASS_WORDS:] == FILL).all())
    none = read.Pattern("b", "-abc")                                 # lines 3 and 4 cannot spell it: no entry, a mass of -inf, no flag
    got, masses, host, _ = _run(dev, x, none, 8, 8)
    for b in (3, 4):
        assert got[b].entries == [] and got[b].flag == 0 and masses[b] == read.PatternMass(-math.inf, 0)
        assert host[b, 0] == 0 and host[b, 1] == 0 and bool((host[b, 2:] == FILL).all())
    assert [c for c, _ in got[0].entries] == [[2]] and masses[0].mass > -math.inf


def test_strided_logits_and_scattered_rows(dev):
    from tatt_amd import read
    case = PATTERN_CASES[2]
    T, B, C, beam, nbest, s, seed, spec, alphabet = case
    x, pat, want, wide = pattern_case(case)
    bar, mbar, _, _ = pattern_bars(T, pat.n_states, C, want, wide)
    big = torch.zeros(T, B + 3, 64, device=dev)                      # a strided view, neither packed nor at the start of its buffer
    big[:, 1:B + 2, 3:3 + C] = torch.cat([x, x[:, :1]], 1).to(dev)   # (line B: line 0 again, sent to row -1)
    view = big[:, 1:B + 2, 3:3 + C]
    cap, n_rows = T + 3, B + 3                                       # an odd cap: one pad word per entry
    order = [n_rows - 2 - b for b in range(B)] + [-1]                # reverse order into a larger record
    width = read.pattern_record_words(cap, nbest)
    at = read.beam_record_words(cap, nbest)
    rec = torch.full((n_rows, width + 5), FILL, dtype=torch.int32, device=dev)
    idx = torch.tensor(order, dtype=torch.int32).to(dev)
    read.ctc_beam_pattern_read(view, pat, idx, rec, cap, beam, nbest)
    read.ctc_pattern_mass(view, pat, idx, rec[:, at:])               # the mass behind the beam row, as the reader lays it
    host = rec.cpu()
    for r in range(n_rows):
        if r not in order:
            assert bool((host[r] == FILL).all()), r                  # untouched rows keep their fill
    assert bool((host[:, width:] == FILL).all())                     # the canary beyond the stated words
    rows = host[[order[b] for b in range(B)]]
    got, masses = read.parse_beam_records(rows[:, :at].contiguous(), cap, nbest), read.parse_pattern_mass(rows[:, at:])
    for g, m, w in zip(got, masses, want):
        assert [c for c, _ in g.entries] == [c for c, _ in w.entries] and g.flag == m.flag == 0
        assert all(abs(a[1] - c[1]) <= bar for a, c in zip(g.entries, w.entries)) and _mass_err(m, w) <= mbar
    packed, pmass, _, _ = _run(dev, x, pat, beam, nbest)
    assert [g.entries for g in got] == [p.entries for p in packed] and masses == pmass       # the very same float64 values either way
    rec.fill_(FILL)
    none = torch.tensor([-1, n_rows, -5, 2 ** 30], dtype=torch.int32).to(dev)
    read.ctc_beam_pattern_read(view, pat, none, rec, cap, beam, nbest)
    read.ctc_pattern_mass(view, pat, none, rec[:, at:])
    assert bool((rec == FILL).all())                                 # no index inside 0 .. n_rows - 1: nothing is written


def test_the_entries_refuse_without_launching(dev):
    from tatt_amd import ops, read
    lim = read.pattern_limits()
    assert lim == {"steps": 256, "classes": 64, "states": 64, "beam": 16}
    T, B, C = 5, 2, 7
    x = torch.randn(300, B, 70, device=dev)                          # (large enough for every geometry asked for below)
    cap = lim["steps"] + 1
    rec = torch.full((4, read.beam_record_words(cap, 16)), FILL, dtype=torch.int32, device=dev)
    out = torch.full((4, 8), FILL, dtype=torch.int32, device=dev)
    idx = torch.arange(B, dtype=torch.int32).to(dev)
    pat = read.Pattern(".{63}", WIDE)                                # 64 states over 64 classes: a table of 4096 bytes
    table, accept = pat.device(dev)

    def beam(**kw):
        a = dict(x=ops.P(x), T=T, B=B, C=C, beam=8, nbest=4, tab=ops.P(table), acc=ops.P(accept), S=1, idx=ops.P(idx), rec=ops.P(rec),
                 rows=4, cap=cap, st=rec.stride(0))
        a.update(kw)
        return ops.LIB.tatt_ctc_beam_pattern_read(a["x"], *x.stride(), a["T"], a["B"], a["C"], a["beam"], a["nbest"], a["tab"], a["acc"],
                                                  a["S"], a["idx"], a["rec"], a["rows"], a["cap"], a["st"], ops.stream())

    def mass(**kw):
        a = dict(x=ops.P(x), T=T, B=B, C=C, tab=ops.P(table), acc=ops.P(accept), S=1, idx=ops.P(idx), out=ops.P(out), rows=4, st=out.stride(0))
        a.update(kw)
        return ops.LIB.tatt_ctc_pattern_mass(a["x"], *x.stride(), a["T"], a["B"], a["C"], a["tab"], a["acc"], a["S"], a["idx"], a["out"],
                                             a["rows"], a["st"], ops.stream())
    shared = ({"T": lim["steps"] + 1}, {"T": 0}, {"C": lim["classes"] + 1}, {"C": 0}, {"S": lim["states"] + 1}, {"S": 0}, {"B": 0},
              {"rows": 0}, {"x": None}, {"idx": None}, {"tab": None}, {"acc": None})
    for kw in shared + ({"beam": lim["beam"] + 1, "nbest": 1}, {"nbest": 9}, {"nbest": 0}, {"cap": T - 1},
                        {"st": read.beam_record_words(cap, 4) - 1}, {"rec": None}):
        assert beam(**kw) == 1, kw
    for kw in shared + ({"st": read.PATTERN_MASS_WORDS - 1}, {"out": None}):
        assert mass(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((rec == FILL).all()) and bool((out == FILL).all())   # refused: nothing is written
    # the limits themselves are taken: 256 steps, 64 classes, 64 states, 16 entries
    assert beam(T=lim["steps"], C=lim["classes"], S=lim["states"], beam=lim["beam"], nbest=16) == 0
    assert mass(T=lim["steps"], C=lim["classes"], S=lim["states"]) == 0
    tight = torch.full((4, read.PATTERN_MASS_WORDS), FILL, dtype=torch.int32, device=dev)      # rows of exactly the stated words
    assert mass(out=ops.P(tight), st=read.PATTERN_MASS_WORDS) == 0
    torch.cuda.synchronize()
    assert int(rec[0, 1]) == 0 and 0 <= int(rec[0, 0]) <= 16 and int(out[0, 2]) == 0 and bool((out[:, 4:] == FILL).all())
    assert bool((tight[:2, 2:] == 0).all()) and bool((tight[2:] == FILL).all())
    with pytest.raises(ValueError):
        read.ctc_beam_pattern_read(x[:T, :, :C], read.Pattern("a", "-abc"), idx, rec, cap, beam=17, nbest=1)
    with pytest.raises(ValueError):
        read.ctc_beam_pattern_read(x[:T, :, :C], read.Pattern("a", "-abc"), idx, rec, T - 1)
    with pytest.raises(ValueError):
        read.ctc_beam_pattern_read(x[:T, :, :C], pat, idx, rec, cap)            # 64 classes against 7
    with pytest.raises(ValueError):
        read.ctc_pattern_mass(x[:T, :, :C], pat, idx, out)
    with pytest.raises(ValueError):
        read.ctc_pattern_mass(x[:T, :, :C], read.Pattern("a", "-abc"), idx, out[:, :3])
    with pytest.raises(ValueError):
        read.ctc_pattern_mass(x[:T, :, :C], "a", idx, out)


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
SOURCES = ((16, 64), (16, 72), (16, 76))                             # rw 100, 120, 120: a bucket of one line and a bucket of two


@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


def test_line_reader_and_super_resolver_with_a_pattern(dev, crnn):
    """every PatternReading equals the specifications run on the reader's own logits (kept, copied to the host): strings exactly, logp
    and mass within the bars of those logits; the images byte for byte those without the keyword; a reader without pattern= writes the
    records of before"""
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    pat = read.Pattern(PLATE)
    before = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_decode="beam", read_beam=8, read_nbest=4)
    up = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_decode="beam", read_beam=8, read_nbest=4,
                       read_pattern=PLATE)
    assert isinstance(up.reader.pattern, read.Pattern) and up.reader.pattern.n_states == 8 and before.reader.pattern is None
    pb, pp = before(imgs), up(imgs)
    (images_b, _), (images, texts) = pb.result(), pp.result()
    _same(images, images_b)
    _same(images, SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result())
    assert all(isinstance(r, read.PatternReading) for r in pp.readings()) and texts == [r.text for r in pp.readings()]

    # the reader alone on the very bytes the caller got back, with the launch census of a call
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    reader = read.LineReader(crnn, batch_size=8, keep_logits=True, decode="beam", beam=8, nbest=4, pattern=pat)
    names = ("ctc_beam_pattern_read", "ctc_pattern_mass", "ctc_beam_read", "ctc_greedy_read")
    census, real = {n: 0 for n in names}, {n: getattr(read, n) for n in names}

    def counted(name, fn):
        def run(*a):
            census[name] += 1
            return fn(*a)
        return run
    for n in names:
        setattr(read, n, counted(n, real[n]))
    try:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                      # nothing waits for the device before result()
        try:
            pending = reader.read(buf, rows, 2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        for n in names:
            setattr(read, n, real[n])
    assert census == {"ctc_beam_pattern_read": 2, "ctc_pattern_mass": 2, "ctc_beam_read": 0, "ctc_greedy_read": 0}
    readings = pending.result()
    assert [idx for idx, _ in pending.logits] == [[0], [1, 2]]
    assert [(r.rw, r.squeezed) for r in readings] == [(100, False), (120, False), (120, False)]
    assert pending.texts() == [r.text for r in readings]
    for idx, lg in pending.logits:
        host = lg.cpu()
        T, _, C = host.shape
        want = read.ctc_beam_pattern_read_host(host, pat, 8, 4, details=True)
        wide = read.ctc_beam_pattern_read_host(host, pat, 8, 4, real=np.longdouble)
        bar, mbar, _, _ = pattern_bars(T, pat.n_states, C, want, wide)
        for j, i in enumerate(idx):
            w, r = want[j], readings[i]
            err = max([abs(a[1] - b[1]) for a, b in zip(r.alternatives, w.entries)], default=0.0)
            print("line %d: logp bar %.3g, device - specification %.3g; mass bar %.3g, device - specification %.3g; margin %.3g, "
                  "entries %d" % (i, bar, err, mbar, abs(r.mass - w.mass), w.margin, len(w.entries)))
            assert w.flag == 0 and w.margin > 100 * bar
            assert [t for t, _, _ in r.alternatives] == ["".join(READER[c] for c in cl) for cl, _ in w.entries] and err <= bar
            assert abs(r.mass - w.mass) <= mbar and all(pat.accepts(t) for t, _, _ in r.alternatives)
            if r.alternatives:
                assert (r.text, r.logp, r.posterior) == r.alternatives[0] and r.posterior == math.exp(r.logp - r.mass)
                assert all(0.0 < p <= 1.0 + 1e-12 for _, _, p in r.alternatives)
            else:
                assert r.text == "" and math.isnan(r.logp) and math.isnan(r.posterior)
    assert texts == [r.text for r in readings]                       # what SuperResolver read off the same lines
    assert [[t for t, _, _ in r.alternatives] for r in pp.readings()] == [[t for t, _, _ in r.alternatives] for r in readings]

    # without the keyword: the record buffer of before, word for word what tatt_ctc_beam_read writes for the kept logits
    plain = read.LineReader(crnn, batch_size=8, keep_logits=True, decode="beam", beam=8, nbest=4)
    p = plain.read(buf, rows, 2)
    p.result()
    cap = 120 // 4 + 1
    assert tuple(p._host.shape) == (3, read.beam_record_words(cap, 4))
    again = torch.full_like(p._host, FILL).to(dev)
    for idx, lg in p.logits:
        read.ctc_beam_read(lg, torch.tensor(idx, dtype=torch.int32).to(dev), again, cap, 8, 4)
    es = read.beam_entry_words(cap)
    for r in range(3):                                               # (words beyond a row's entries are left as they were)
        n = int(p._host[r, 0])
        assert n >= 1 and torch.equal(p._host[r, :2 + n * es], again.cpu()[r, :2 + n * es])


def test_scene_readings_with_a_pattern_and_the_refusals(dev, crnn):
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    from tests.test_scene_device_gpu import BOXES
    gen = _generator(dev)
    up = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn, read_decode="beam", read_beam=4, read_nbest=2,
                       read_pattern=r"[a-z]{1,3}\d?")
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn)
    scene = _img(60, 48, 160, 1)
    p, q = up.scene(scene, BOXES, 2), plain.scene(scene, BOXES, 2)
    _same([p.result()], [q.result()])
    rs = p.readings()
    assert len(rs) == len(BOXES) and all(isinstance(r, read.PatternReading) and len(r.alternatives) <= 2 for r in rs)
    assert p.texts() == [r.text for r in rs] and [(r.rw, r.squeezed) for r in rs] == [(g.rw, g.squeezed) for g in q.readings()]
    assert all(r.mass <= 1e-12 and not math.isnan(r.mass) for r in rs)
    assert all(up.reader.pattern.accepts(t) and lp <= r.mass + 1e-9 for r in rs for t, lp, _ in r.alternatives)
    with pytest.raises(ValueError, match="decode='beam'"):
        SuperResolver(gen, reader=crnn, read_pattern="a")            # the default decoding is greedy
    with pytest.raises(ValueError, match="decode='beam'"):
        read.LineReader(crnn, decode="lexicon", lexicon=["a"], pattern="a")
    lm = read.CharLM(np.log(np.full((37, 37), 1.0 / 37)))
    with pytest.raises(ValueError, match="do not go together"):
        read.LineReader(crnn, decode="beam", lm=lm, pattern="a")
    with pytest.raises(ValueError, match="64 classes, the CRNN emits 37"):
        read.LineReader(crnn, decode="beam", pattern=read.Pattern("a", WIDE))
    with pytest.raises(ValueError, match="65 states"):
        read.LineReader(crnn, decode="beam", pattern=".{64}")
    with pytest.raises(ValueError, match="reader=crnn"):
        SuperResolver(gen, read_pattern="a")
