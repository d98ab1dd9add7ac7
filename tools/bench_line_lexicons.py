"""Per-line lexicons beside the one-list path (csrc/ctclexp.hip, csrc/ctclex.hip): the launches alone on given logits, and
`tatt_amd.read.LineReader` with decode="lexicons" beside "greedy" and "lexicon", in one process, alternating.  Reports only (one JSON
line); asserts nothing but that the pair launch wrote the one-list path's bits and every line got a word.  The library must be built
(`python -m tatt_amd.build`); the tool does not build it.

    timeout -k 10 600 python tools/bench_line_lexicons.py [--repeats 5] [--calls 20] [--warmup 1] [--out FILE]

Launches alone, on seeded logits (randn * 3, C = 37), every line with a seeded list of its own of words of 3 .. 12 characters, no word
shared between lines: (T, n) = (26, 48) and (256, 16) with 50 words per line, and `skew`: (26, 48) with one line of 1,000 words and the
rest 50.  `pairs`: the ONE tatt_ctc_lexicon_score_pairs launch on the tables of `LineLexicons.pack`; `select_rows`: the
tatt_ctc_lexicon_select_rows launch (nbest 4); BESIDE them `union`: the tatt_ctc_lexicon_score launches on the UNION of the lists (every
line against every word: what the one-list path costs a caller who masks on the host) and `floor`: the same entry on ONE 50-word
`Lexicon` for all lines (the work of the wanted pairs in the one-list layout); `select`: tatt_ctc_lexicon_select on the floor's scores.
Device time from events around `--calls` calls, microseconds per call; per repeat every candidate runs one such window, in an order that
rotates with the repeat; min / median / max over the repeats.  `pairs_overlaps_floor_*`: whether the two ranges overlap;
`pairs_below_union_*`: whether the whole range of `pairs` lies below `union`'s.
The reader: the 16 lines of tools/bench_read.py's `lines16` case, `LineReader.read(...).result()` with decode="greedy", "lexicon" (one list
of 50 words) and "lexicons" (16 lists of 50 words: handed over as lists, so that every call makes its `LineLexicons`, and
`lexicons_made`: as a `LineLexicons` made once), host time of a window of `--calls // 4` calls that ends in a device synchronise,
milliseconds per call, same alternation; `reader_*_host_ms`: the same window of `read(...)` alone, timed until the last call
returns (the host share of a call: the plan, the tables of the chunks, the enqueueing), the synchronise outside the window.
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


def make_words(K, seed, seen=None):
    rng, out, seen = random.Random(seed), [], set() if seen is None else seen
    while len(out) < K:
        w = "".join(rng.choice("0123456789abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(3, 12)))
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
    from tatt_amd.infer import SuperResolver
    from oracle.fixtures import randomize_state_dict
    from tests.pil_resample_ref import make_image
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    gen.load_state_dict(randomize_state_dict(gen.state_dict()))
    gen = gen.to(dev).eval()
    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    crnn.load_state_dict(randomize_state_dict(crnn.state_dict(), seed=11))
    crnn = crnn.to(dev).eval()
    res = {"bench": "line_lexicons", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
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

    # ---- the launches alone ----
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    for tag, T, n, sizes in (("T26_n48_K50", 26, 48, [50] * 48), ("T256_n16_K50", 256, 16, [50] * 16), ("skew_T26_n48", 26, 48, [1000] + [50] * 47)):
        seen = set()
        lists = [make_words(K, 1000 * T + b, seen) for b, K in enumerate(sizes)]
        lex = read.LineLexicons(lists)
        one, union = read.Lexicon(lists[-1]), read.Lexicon(lex.union)
        tiles, pairs, counts = lex.pack(range(n))
        most = int(counts.max())
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        rec = torch.empty(n, read.lexicon_record_words(4), dtype=torch.int32, device=dev)
        rec_rows = torch.empty(n, read.lexicon_record_words(4), dtype=torch.int32, device=dev)
        codes, table, tiles_d, pairs_d, counts_d = up(lex.codes), up(lex.table), up(tiles), up(pairs), up(counts)
        s_pairs = torch.empty(n, most, dtype=torch.float64, device=dev)
        s_union = torch.empty(n, len(union), dtype=torch.float64, device=dev)
        s_floor = torch.empty(n, len(one), dtype=torch.float64, device=dev)
        fns = {"pairs": lambda: read.ctc_lexicon_score_pairs(x, codes, lex.n_codes, table, tiles_d, pairs_d, counts_d, s_pairs, most),
               "select_rows": lambda: read.ctc_lexicon_select_rows(s_pairs, counts_d, index, rec_rows, 4),
               "union": lambda: read.ctc_lexicon_score(x, union, s_union),
               "floor": lambda: read.ctc_lexicon_score(x, one, s_floor),
               "select": lambda: read.ctc_lexicon_select(s_floor, index, rec, 4)}
        fns["pairs"]()                                               # (the selects run on scores from their first window on)
        fns["floor"]()
        times = alternate(fns, device_window)
        for k in fns:
            res["%s_us_%s" % (k, tag)] = span(times[k])
        res["tables_%s" % tag] = {"tiles": int(len(tiles)), "pairs": int(len(pairs)), "union": len(lex.union),
                                  "union_classes": union.counts, "floor_classes": one.counts}
        res["pairs_overlaps_floor_%s" % tag] = bool(min(times["pairs"]) <= max(times["floor"]) and min(times["floor"]) <= max(times["pairs"]))
        res["pairs_below_union_%s" % tag] = bool(max(times["pairs"]) < min(times["union"]))
        # the last line's list is the floor's lexicon: the pair launch wrote its bits
        assert torch.equal(s_pairs[n - 1, :50].contiguous().view(torch.int64), s_floor[n - 1].contiguous().view(torch.int64))
        got = read.parse_lexicon_records(rec_rows.cpu(), 4)
        assert all(g.flag == 0 and g.entries for g in got)

    # ---- the reader under the three decodings ----
    rng = np.random.default_rng(7)
    keep = SuperResolver(gen, batch_size=48, long_lines=True, keep_sr=True)
    imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * 4)]
    p = keep(imgs)
    pending = keep.exporter.lines(p.sr, p.lines, 2)
    buf, rows = pending.line_canvases
    buf = buf.clone()
    seen = set()
    lists = [make_words(50, 77 + b, seen) for b in range(16)]
    readers = {"greedy": read.LineReader(crnn, batch_size=48), "lexicon": read.LineReader(crnn, batch_size=48, decode="lexicon", lexicon=lists[0]),
               "lexicons": read.LineReader(crnn, batch_size=48, decode="lexicons")}
    readers["lexicons_made"] = readers["lexicons"]                   # the same reader, handed a LineLexicons made once
    calls = max(1, a.calls // 4)

    def host_window(fn):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    def enqueue_window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        t = (time.perf_counter() - t0) * 1e3 / calls
        torch.cuda.synchronize()
        return t
    kw = {"greedy": {}, "lexicon": {}, "lexicons": {"lexicons": lists}, "lexicons_made": {"lexicons": read.LineLexicons(lists)}}
    fns = {k: (lambda r=r, k=k: r.read(buf, rows, 2, **kw[k]).result()) for k, r in readers.items()}
    first = {k: fn() for k, fn in fns.items()}
    assert all(len(v) == 16 for v in first.values()) and all(r.alternatives and r.text in lists[i] for i, r in enumerate(first["lexicons"]))
    assert first["lexicons_made"] == first["lexicons"]
    res["lines"] = len(rows)
    times = alternate(fns, host_window)
    for k in fns:
        res["reader_%s_ms" % k] = span(times[k], 3)
    res["reader_lexicons_overlaps_lexicon"] = bool(min(times["lexicons"]) <= max(times["lexicon"]) and min(times["lexicon"]) <= max(times["lexicons"]))
    host = alternate({k: (lambda k=k: readers[k].read(buf, rows, 2, **kw[k])) for k in ("lexicons", "lexicons_made", "greedy")},
                     enqueue_window)
    for k in host:
        res["reader_%s_host_ms" % k] = span(host[k], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
