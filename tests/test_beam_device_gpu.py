"""The CTC prefix beam search on the GPU (csrc/ctcbeam.hip; read.ctc_beam_read, read.LineReader(decode="beam"),
infer.SuperResolver(read_decode="beam")).  Yardstick: the host specification read.ctc_beam_read_host in float64, itself held to brute force
by tests/test_beam.py.  Strings, lengths and order are exact; logp within a bar that is measured per case FROM THE SPECIFICATION ALONE:
4 x the distance of the float64 specification from the same specification run in np.longdouble, plus T x 2^-52 x max |logp| (one rounding
of the running sum per step).  The ids of a row are compared only if its float64 selection margin exceeds 100 x the bar, and no row may
be left out.  Shapes: tests/test_beam.py CASES, the smallest at which each limit and each path of the kernel is met."""
import math

import numpy as np
import pytest
import torch

from oracle.fixtures import randomize_state_dict
from tests.test_beam import CASES, beam_case, beam_logits, brute_force
from tests.test_lines_device_gpu import LR, _generator, _img, _same
from tests.test_read_device_gpu import _upload

pytestmark = pytest.mark.gpu
_wide = {}


def _bar(case):
    """-> (the bar on logp, the distance float64 - longdouble of the specification) of a case; strings must agree between the two"""
    if case not in _wide:
        from tatt_amd import read
        T, B, C, beam, nbest, s, seed = case
        x, want = beam_case(case)
        wide = read.ctc_beam_read_host(x, beam, nbest, real=np.longdouble)
        dist = top = 0.0
        for w, l in zip(want, wide):
            assert [c for c, _ in w.entries] == [c for c, _ in l.entries]
            dist = max(dist, max(abs(float(np.longdouble(a[1]) - b[1])) for a, b in zip(w.entries, l.entries)))
            top = max(top, max(abs(a[1]) for a in w.entries))
        _wide[case] = (4 * dist + T * 2.0 ** -52 * top, dist)
    return _wide[case]


def _run(dev, x, beam, nbest, cap=None):
    """one launch on contiguous logits, rows in input order -> (BeamDecoded per image, the record on the host)"""
    from tatt_amd import read
    T, B, C = x.shape
    cap = T if cap is None else cap
    rec = torch.full((B, read.beam_record_words(cap, nbest)), -77, dtype=torch.int32, device=dev)
    read.ctc_beam_read(x.to(dev), torch.arange(B, dtype=torch.int32).to(dev), rec, cap, beam, nbest)
    host = rec.cpu()
    return read.parse_beam_records(host, cap, nbest), host


def _compare(got, want, bar, what):
    """strings, lengths, order exactly; logp within the bar -> the largest |logp - specification|"""
    worst = 0.0
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert w.margin > 100 * bar, "%s row %d: margin %.3g against a bar of %.3g: take another seed" % (what, b, w.margin, bar)
        assert g.flag == w.flag == 0 and [c for c, _ in g.entries] == [c for c, _ in w.entries], (what, b, g.entries, w.entries)
        worst = max(worst, max(abs(a[1] - c[1]) for a, c in zip(g.entries, w.entries)))
    return worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d-B%d-C%d-beam%d-nbest%d-s%g" % c[:6])
def test_ctc_beam_read_equals_the_specification(dev, case):
    """Measured on an MI355X: see the README, section "Reading lines" (the bar and the distance of every case)."""
    from tatt_amd import read
    T, B, C, beam, nbest, s, seed = case
    x, want = beam_case(case)
    bar, dist = _bar(case)
    got, host = _run(dev, x, beam, nbest)
    worst = _compare(got, want, bar, "case %s" % (case,))
    print("case %s: bar %.3g (float64 - longdouble of the specification %.3g), device - specification %.3g, smallest margin %.3g, "
          "rows with a re-entry %d" % (case[:6], bar, dist, worst, min(w.margin for w in want), sum(w.reentry for w in want)))
    assert worst <= bar, (worst, bar)
    es = read.beam_entry_words(T)
    for b, g in enumerate(got):                                      # the row as the header states it
        assert host[b, 0] == len(g.entries) and host[b, 1] == 0
        for i, (c, _) in enumerate(g.entries):
            e = host[b, 2 + i * es:2 + (i + 1) * es]
            assert e[2] == len(c) and e[3] == 0 and bool((e[4 + len(c):] == -1).all())
        assert bool((host[b, 2 + len(g.entries) * es:] == -77).all())        # entries that do not exist are not written
    if beam >= 16 and C ** T <= 81:                                  # the exhaustive shape: every string, as brute force orders them
        for b, g in enumerate(got):
            exact = sorted(brute_force(x[:, b]).items(), key=lambda kv: -kv[1])
            assert [tuple(c) for c, _ in g.entries] == [k for k, _ in exact]
            assert max(abs(a[1] - w) for a, (_, w) in zip(g.entries, exact)) <= 1e-14 + bar


def test_exact_ties_go_to_the_lower_key(dev):
    """all logits equal (tests/test_beam.py has the order by hand): candidates of equal value in several lanes, where the lowest lane
    does not hold the lowest key; equal values stay equal on the device because tied candidates go through the same operations"""
    from tatt_amd import read
    x = torch.zeros(2, 2, 4)
    want = read.ctc_beam_read_host(x, 5, 5)
    got, _ = _run(dev, x, 5, 5)
    for g, w in zip(got, want):
        assert [c for c, _ in g.entries] == [c for c, _ in w.entries] == [[1], [2], [3], [], [1, 2]]
        assert max(abs(a[1] - b[1]) for a, b in zip(g.entries, w.entries)) <= 4 * 2.0 ** -52 * 3   # (two steps, |logp| < 3)
        assert g.entries[0][1] == g.entries[1][1] == g.entries[2][1] and g.entries[3][1] == g.entries[4][1]


def test_strided_logits_and_scattered_rows(dev):
    from tatt_amd import read
    case = CASES[2]
    T, B, C, beam, nbest, s, seed = case
    x, want = beam_case(case)
    wide = torch.zeros(T, B + 3, 64, device=dev)                     # a strided view, neither packed nor at the start of its buffer
    wide[:, 1:B + 2, 3:3 + C] = torch.cat([x, x[:, :1]], 1).to(dev)  # (image B: image 0 again, sent to row -1)
    view = wide[:, 1:B + 2, 3:3 + C]
    assert view.stride() == ((B + 3) * 64, 64, 1) and view.storage_offset() == 67
    cap, n_rows = T + 3, B + 3                                       # an odd cap: one pad word per entry
    order = [n_rows - 2 - b for b in range(B)] + [-1]                # reverse order into a larger record
    width = read.beam_record_words(cap, nbest)
    rec = torch.full((n_rows, width + 5), -77, dtype=torch.int32, device=dev)
    read.ctc_beam_read(view, torch.tensor(order, dtype=torch.int32).to(dev), rec, cap, beam, nbest)
    host = rec.cpu()
    for r in range(n_rows):
        if r not in order:
            assert bool((host[r] == -77).all()), r                   # untouched rows keep their fill
    assert bool((host[:, width:] == -77).all())
    rows = host[[order[b] for b in range(B)]][:, :width].contiguous()
    got = read.parse_beam_records(rows, cap, nbest)
    worst = _compare(got, want, _bar(case)[0], "scattered")
    assert worst <= _bar(case)[0]
    plain, _ = _run(dev, x, beam, nbest)
    assert [g.entries for g in got] == [p.entries for p in plain]    # the very same float64 values by either way in
    rec.fill_(-77)
    read.ctc_beam_read(view, torch.tensor([-1, n_rows, -5, 2 ** 30], dtype=torch.int32).to(dev), rec, cap, beam, nbest)
    assert bool((rec == -77).all())                                  # no index inside 0 .. n_rows - 1: nothing is written


def test_flagged_lines_beside_clean_ones(dev):
    from tatt_amd import read
    inf = float("inf")
    x = beam_logits(6, 6, 4, 3.0, 40)
    x[2, 1, 3] = float("nan")
    x[5, 2, 0] = inf
    x[:, 3, 0] = -inf                                                # no blank, classes 1 and 3 only
    x[:, 3, 2] = -inf
    x[:, 4, 1:3] = -inf                                              # the blank and 3: four strings, a beam shorter than `beam`
    x[3, 5] = -inf                                                   # a step without a finite logit
    want = read.ctc_beam_read_host(x, 8, 8)
    assert [w.flag for w in want] == [0, 1, 1, 0, 0, 1] and [len(w.entries) for w in want] == [8, 0, 0, 8, 4, 0]
    got, host = _run(dev, x, 8, 8)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.flag == w.flag and [c for c, _ in g.entries] == [c for c, _ in w.entries], (b, g, w)
        assert all(abs(a[1] - c[1]) <= 1e-12 for a, c in zip(g.entries, w.entries))          # (6 steps: far inside any bar of CASES)
        if w.flag:
            assert host[b, 0] == 0 and host[b, 1] == 1 and bool((host[b, 2:] == -77).all())


def test_the_entry_refuses_without_launching(dev):
    from tatt_amd import ops, read
    lim = read.beam_limits()
    T, B, C = 5, 2, 7
    x = torch.randn(300, B, 70, device=dev)                          # (large enough for every geometry asked for below)
    cap = lim["steps"] + 1
    rec = torch.full((4, read.beam_record_words(cap, 16)), -77, dtype=torch.int32, device=dev)
    idx = torch.arange(B, dtype=torch.int32).to(dev)

    def run(**kw):
        a = dict(x=ops.P(x), T=T, B=B, C=C, beam=8, nbest=4, idx=ops.P(idx), rec=ops.P(rec), rows=4, cap=cap, st=rec.stride(0))
        a.update(kw)
        return ops.LIB.tatt_ctc_beam_read(a["x"], *x.stride(), a["T"], a["B"], a["C"], a["beam"], a["nbest"], a["idx"], a["rec"],
                                          a["rows"], a["cap"], a["st"], ops.stream())
    for kw in ({"T": lim["steps"] + 1}, {"T": 0}, {"C": lim["classes"] + 1}, {"C": 0}, {"beam": lim["beam"] + 1, "nbest": 1},
               {"nbest": 9}, {"nbest": 0}, {"beam": 0, "nbest": 0}, {"cap": T - 1}, {"B": 0}, {"rows": 0},
               {"st": read.beam_record_words(cap, 4) - 1}, {"x": None}, {"idx": None}, {"rec": None}):
        assert run(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool((rec == -77).all())
    assert run(st=read.beam_record_words(cap, 4)) == 0 and run(T=lim["steps"], C=lim["classes"], beam=lim["beam"], nbest=16) == 0
    torch.cuda.synchronize()
    assert int(rec[0, 1]) == 0 and 1 <= int(rec[0, 0]) <= 16
    with pytest.raises(ValueError):
        read.ctc_beam_read(x[:T, :, :C], idx, rec, cap, beam=17, nbest=1)
    with pytest.raises(ValueError):
        read.ctc_beam_read(x[:T, :, :C], idx, rec, T - 1)
    with pytest.raises(ValueError):
        read.ctc_beam_read(x[:T, :, :C], idx, rec[:, :20], cap)


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
SOURCES = ((16, 64), (16, 72), (16, 76))                             # rw 100, 120, 120: a bucket of one line and a bucket of two


@pytest.fixture(scope="module")
def crnn(dev):
    import tatt_amd
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=11))
    return c.to(dev).eval()


def test_line_reader_and_super_resolver_with_a_beam(dev, crnn):
    """every BeamReading equals the specification run on the reader's own logits (kept, copied to the host): strings exactly, logp within
    the bar of those logits; rw and squeezed as the greedy reader gives them; the images byte for byte those without the keywords"""
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    gen = _generator(dev)
    imgs = [_img(90 + i, hs, ws) for i, (hs, ws) in enumerate(SOURCES)]
    greedy = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn)
    up = SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True, reader=crnn, read_decode="beam", read_beam=8, read_nbest=4)
    assert (up.reader.decode, up.reader.beam, up.reader.nbest, greedy.reader.decode) == ("beam", 8, 4, "greedy")
    pg, pb = greedy(imgs), up(imgs)
    (images_g, texts_g), (images, texts) = pg.result(), pb.result()
    _same(images, images_g)
    _same(images, SuperResolver(gen, batch_size=8, lr_size=LR, long_lines=True)(imgs).result())
    want_rw = [(r.rw, r.squeezed) for r in pg.readings()]
    assert want_rw == [(100, False), (120, False), (120, False)]
    assert all(isinstance(r, read.BeamReading) for r in pb.readings()) and texts == [r.text for r in pb.readings()]

    # the reader alone on the very bytes the caller got back, with the launch census of a call
    buf, rows = _upload(dev, [np.asarray(im) for im in images])
    reader = read.LineReader(crnn, batch_size=8, keep_logits=True, decode="beam", beam=8, nbest=4)
    census, real = {"beam": 0, "greedy": 0}, (read.ctc_beam_read, read.ctc_greedy_read)

    def counted(name, fn):
        def run(*a):
            census[name] += 1
            return fn(*a)
        return run
    read.ctc_beam_read, read.ctc_greedy_read = counted("beam", real[0]), counted("greedy", real[1])
    try:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                      # nothing waits for the device before result()
        try:
            pending = reader.read(buf, rows, 2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        read.ctc_beam_read, read.ctc_greedy_read = real
    assert census == {"beam": 2, "greedy": 0}                        # one launch per bucket chunk, in place of the greedy one
    readings = pending.result()
    assert [idx for idx, _ in pending.logits] == [[0], [1, 2]]
    assert [(r.rw, r.squeezed) for r in readings] == want_rw and pending.texts() == [r.text for r in readings]
    d2a = "-0123456789abcdefghijklmnopqrstuvwxyz"
    for idx, lg in pending.logits:
        host = lg.cpu()
        want = read.ctc_beam_read_host(host, 8, 4, details=True)
        wide = read.ctc_beam_read_host(host, 8, 4, real=np.longdouble)
        for j, i in enumerate(idx):
            w, r = want[j], readings[i]
            dist = max(abs(float(np.longdouble(a[1]) - b[1])) for a, b in zip(w.entries, wide[j].entries))
            bar = 4 * dist + host.shape[0] * 2.0 ** -52 * max(abs(a[1]) for a in w.entries)
            err = max(abs(a[1] - b[1]) for a, b in zip(r.alternatives, w.entries))
            print("line %d: bar %.3g, device - specification %.3g, margin %.3g" % (i, bar, err, w.margin))
            assert w.flag == 0 and w.margin > 100 * bar
            assert [t for t, _ in r.alternatives] == ["".join(d2a[c] for c in cl) for cl, _ in w.entries] and err <= bar
            assert (r.text, r.logp) == r.alternatives[0] and len(r.alternatives) == 4
    assert texts == [r.text for r in readings]                       # what SuperResolver read off the same lines
    assert [[t for t, _ in r.alternatives] for r in pb.readings()] == [[t for t, _ in r.alternatives] for r in readings]


def test_scene_readings_with_a_beam(dev, crnn):
    from tatt_amd import read
    from tatt_amd.infer import SuperResolver
    from tests.test_quads_device_gpu import QUADS
    from tests.test_scene_device_gpu import BOXES
    gen = _generator(dev)
    up = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn, read_decode="beam", read_beam=4, read_nbest=2)
    plain = SuperResolver(gen, batch_size=4, lr_size=LR, stride=32, reader=crnn)
    for scene, regions, run, run_plain in ((_img(60, 48, 160, 1), BOXES, up.scene, plain.scene),
                                           (_img(61, 97, 211, 1), QUADS, up.scene_quads, plain.scene_quads)):
        p, q = run(scene, regions, 2), run_plain(scene, regions, 2)
        _same([p.result()], [q.result()])
        rs = p.readings()
        assert len(rs) == len(regions) and all(isinstance(r, read.BeamReading) and 1 <= len(r.alternatives) <= 2 for r in rs)
        assert p.texts() == [r.text for r in rs] and [(r.rw, r.squeezed) for r in rs] == [(g.rw, g.squeezed) for g in q.readings()]
        assert all(r.logp <= 0.0 and not math.isnan(r.logp) for r in rs)
    with pytest.raises(ValueError, match="decode"):
        SuperResolver(gen, reader=crnn, read_decode="best")
    with pytest.raises(ValueError, match="nbest <= beam"):
        SuperResolver(gen, reader=crnn, read_decode="beam", read_beam=17)
