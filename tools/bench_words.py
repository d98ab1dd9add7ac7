"""Word segmentation beside the greedy, the beam and the lexicon decoding (csrc/ctcwords.hip, csrc/read.hip, csrc/ctcbeam.hip,
csrc/ctclex.hip): the launches alone on given logits, and `tatt_amd.read.LineReader` under the four decodings, in one process,
alternating.  Reports only (one JSON line); asserts nothing but that every line was read.

    timeout -k 10 600 python tools/bench_words.py [--repeats 5] [--calls 20] [--warmup 1] [--out FILE]

Launches alone, on seeded logits (randn * 3, C = 37) and a seeded lexicon of K words of 3 .. 7 characters (1000 of them fill 16000 of
the 16384 packed lanes of the words launch), at (T, n, K) = (26, 48, 50), (26, 48, 1000) and (256, 16, 1000): `words`:
tatt_ctc_words_read, `words_lp`: the same launch writing lp_out, `greedy`, `beam8` (nbest 4), `lexicon`: the tatt_ctc_lexicon_score
launches + tatt_ctc_lexicon_select (nbest 4), and `forward`: the chunk's CRNN forward (`LineReader.forward` on an (n, 1, 32, 4 (T - 1))
input) -- device time from events around `--calls` calls, microseconds per call; per repeat every candidate runs one such window, in an
order that rotates with the repeat; min / median / max over the repeats.  `words_us_per_step_*`: the words range divided by T.
`words_vs_<other>_*`: "below" / "above" where the two ranges are disjoint, "overlap" otherwise.
The reader: the 16 lines of tools/bench_read.py's `lines16` case (four each of 128, 300, 600 and 1200 columns at 40 rows, blended once),
`LineReader.read(...).result()` with decode="greedy", "beam" (beam 8, nbest 4), "lexicon" (K = 1000, nbest 4) and "words" (K = 1000),
host time of a window of `--calls // 4` calls that ends in a device synchronise, milliseconds per call, same alternation.
TSRN and CRNN with seeded weights; batch_size 48."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def make_words(K, seed):
    rng, out, seen = random.Random(seed), [], set()
    while len(out) < K:
        w = "".join(rng.choice("0123456789abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(3, 7)))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from PIL import Image
    import tatt_amd
    from tatt_amd import read
    from tatt_amd.build import build
    from tatt_amd.infer import SuperResolver
    from oracle.fixtures import randomize_state_dict
    from tests.pil_resample_ref import make_image
    build(verbose=False)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    gen.load_state_dict(randomize_state_dict(gen.state_dict()))
    gen = gen.to(dev).eval()
    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    crnn.load_state_dict(randomize_state_dict(crnn.state_dict(), seed=11))
    crnn = crnn.to(dev).eval()
    res = {"bench": "words", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0), "limits": read.words_limits()}
    span = lambda ts, nd=2: {"min": round(min(ts), nd), "median": round(statistics.median(ts), nd), "max": round(max(ts), nd)}

    def alternate(fns, window):
        names = list(fns)
        for k in names:
            for _ in range(a.warmup):
                window(fns[k])
        times = {k: [] for k in names}
        for r in range(a.repeats):
            rot = r % len(names)
            for k in names[rot:] + names[:rot]:
                times[k].append(window(fns[k]))
        return times

    def device_window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    def versus(x, y):
        return "below" if max(x) < min(y) else "above" if min(x) > max(y) else "overlap"

    # ---- the launches alone ----
    reader = read.LineReader(crnn, batch_size=48)
    for T, n, K in ((26, 48, 50), (26, 48, 1000), (256, 16, 1000)):
        lex = read.Lexicon(make_words(K, K))
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        img = torch.rand(n, 1, 32, 4 * (T - 1), generator=torch.Generator().manual_seed(n)).to(dev)
        assert reader.forward(img).shape == (T, n, 37)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        greedy_rec = torch.empty(n, 3 * T + 2, dtype=torch.int32, device=dev)
        beam_rec = torch.empty(n, read.beam_record_words(T, 4), dtype=torch.int32, device=dev)
        lex_rec = torch.empty(n, read.lexicon_record_words(4), dtype=torch.int32, device=dev)
        words_rec = torch.empty(n, read.words_record_words(T), dtype=torch.int32, device=dev)
        scores = torch.empty(n, K, dtype=torch.float64, device=dev)
        lp = torch.empty(n, T, 37, dtype=torch.float64, device=dev)

        def lexicon():
            read.ctc_lexicon_score(x, lex, scores)
            read.ctc_lexicon_select(scores, index, lex_rec, 4)
        fns = {"words": lambda: read.ctc_words_read(x, lex, index, words_rec, T),
               "words_lp": lambda: read.ctc_words_read(x, lex, index, words_rec, T, 0.0, lp),
               "greedy": lambda: read.ctc_greedy_read(x, index, greedy_rec, T),
               "beam8": lambda: read.ctc_beam_read(x, index, beam_rec, T, 8, 4),
               "lexicon": lexicon,
               "forward": lambda: reader.forward(img)}
        times = alternate(fns, device_window)
        tag = "T%d_n%d_K%d" % (T, n, K)
        for k in fns:
            res["%s_us_%s" % (k, tag)] = span(times[k])
        res["words_us_per_step_%s" % tag] = span([t / T for t in times["words"]], 3)
        res["lanes_%s" % tag] = read.words_lanes(lex)
        for k in ("greedy", "beam8", "lexicon", "forward"):
            res["words_vs_%s_%s" % (k, tag)] = versus(times["words"], times[k])
        got = read.parse_words_records(words_rec.cpu(), T)
        assert all(g.flag == 0 and g.words for g in got)
        res["words_per_line_%s" % tag] = round(sum(len(g.words) for g in got) / n, 1)

    # ---- the reader under the four decodings ----
    rng = np.random.default_rng(7)
    keep = SuperResolver(gen, batch_size=48, long_lines=True, keep_sr=True)
    imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * 4)]
    p = keep(imgs)
    pending = keep.exporter.lines(p.sr, p.lines, 2)
    buf, rows = pending.line_canvases
    buf = buf.clone()
    words = make_words(1000, 1000)
    readers = {"greedy": reader, "beam": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4),
               "lexicon": read.LineReader(crnn, batch_size=48, decode="lexicon", lexicon=words, nbest=4),
               "words": read.LineReader(crnn, batch_size=48, decode="words", lexicon=words)}
    calls = max(1, a.calls // 4)

    def host_window(fn):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls
    fns = {k: (lambda r=r: r.read(buf, rows, 2).result()) for k, r in readers.items()}
    first = {k: fn() for k, fn in fns.items()}
    assert all(len(v) == 16 for v in first.values()) and all(r.logp == r.logp for r in first["words"])
    res["lines"] = len(rows)
    times = alternate(fns, host_window)
    for k in fns:
        res["reader_%s_ms" % k] = span(times[k], 3)
    for k in ("greedy", "beam", "lexicon"):
        res["reader_words_vs_%s" % k] = versus(times["words"], times[k])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
