"""Reading against a format (csrc/ctcbeam.hip's pattern instantiation, csrc/ctcpat.hip): the two launches alone beside the plain beam-8
launch and the chunk's forward, and `tatt_amd.read.LineReader(decode="beam")` with and without pattern=, in one process, alternating.
Reports only (one JSON line); asserts nothing but that every line was decoded.

    timeout -k 10 600 python tools/bench_pattern.py [--repeats 5] [--calls 50] [--warmup 1] [--out FILE]

Expectation, stated before any measurement: the constrained search does the plain search's work plus BM byte loads per step from a table
of at most 4 KB, so it should cost about what the language-model fusion costs (some 10 % of the launch) or less, and less where the
format leaves few candidates; the mass is O(T S C) with a wave sum and two scans per live DFA state and step, so it should lie well
below the search for the 8-state plate format and may exceed it for a 64-state format at 256 steps.  The tool prints ranges and whether
they overlap; it promises no ratio.
Launches alone, on seeded logits (randn * 3, C = 37) at (T, n) = (26, 48) and (256, 16), beam 8, nbest 4: `plain` (tatt_ctc_beam_read),
`beam_plate` / `mass_plate` (the plate format [a-z]{2}\\d{2}[a-z]{3}, 8 states) and `beam_s64` / `mass_s64` (.{40,63}, 64 states; at
T = 26 no string of 40 characters has an alignment, so the search ends without entries and the mass is -inf: the cost is still the
kernel's), and `forward`, the recogniser's folded eval forward of that chunk (n lines of width 4 (T - 1)) -- device time from events
around `--calls` launches, microseconds per launch; per repeat every candidate runs one such window, in an order that rotates with the
repeat; min / median / max over the repeats.
The reader: the 16 lines of tools/bench_read.py's `lines16` case, `LineReader.read(...).result()` with decode="beam" (beam 8, nbest 4)
without and with pattern= (the plate format), host time of a window of `--calls // 4` calls that ends in a device synchronise,
milliseconds per call, same alternation.  TSRN and CRNN with seeded weights; batch_size 48.  The library is the one the build left in
the tree (python -m tatt_amd.build)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
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
    res = {"bench": "pattern", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    span = lambda ts, nd=2: {"min": round(min(ts), nd), "median": round(statistics.median(ts), nd), "max": round(max(ts), nd)}
    overlap = lambda p, q: bool(min(p) <= max(q) and min(q) <= max(p))

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

    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    crnn.load_state_dict(randomize_state_dict(crnn.state_dict(), seed=11))
    crnn = crnn.to(dev).eval()
    pats = {"plate": read.Pattern(r"[a-z]{2}\d{2}[a-z]{3}"), "s64": read.Pattern(".{40,63}")}
    res["states"] = {k: p.n_states for k, p in pats.items()}
    plain_reader = read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4)

    # ---- the launches alone ----
    for T, n in ((26, 48), (256, 16)):
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        img = torch.rand(n, 1, 32, 4 * (T - 1), generator=torch.Generator().manual_seed(T)).to(dev)
        assert plain_reader.forward(img).shape == (T, n, 37)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        plain_rec = torch.empty(n, read.beam_record_words(T, 4), dtype=torch.int32, device=dev)
        recs = {k: torch.empty(n, read.pattern_record_words(T, 4), dtype=torch.int32, device=dev) for k in pats}
        at = read.beam_record_words(T, 4)
        fns = {"plain": lambda: read.ctc_beam_read(x, index, plain_rec, T, 8, 4), "forward": lambda: plain_reader.forward(img)}
        for k, p in pats.items():
            fns["beam_" + k] = lambda k=k, p=p: read.ctc_beam_pattern_read(x, p, index, recs[k], T, 8, 4)
            fns["mass_" + k] = lambda k=k, p=p: read.ctc_pattern_mass(x, p, index, recs[k][:, at:])
        times = alternate(fns, device_window)
        for k in fns:
            res["%s_us_T%d_n%d" % (k, T, n)] = span(times[k])
            if k.startswith("beam_"):
                res["%s_overlaps_plain_T%d_n%d" % (k, T, n)] = overlap(times[k], times["plain"])
        assert all(g.flag == 0 and g.entries for g in read.parse_beam_records(plain_rec.cpu(), T, 4))
        for k in pats:
            host = recs[k].cpu()
            assert all(g.flag == 0 for g in read.parse_beam_records(host, T, 4)) and all(m.flag == 0 for m in read.parse_pattern_mass(host[:, at:]))
            res["lines_with_entries_%s_T%d" % (k, T)] = sum(bool(g.entries) for g in read.parse_beam_records(host, T, 4))

    # ---- the reader without and with the format ----
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    gen.load_state_dict(randomize_state_dict(gen.state_dict()))
    gen = gen.to(dev).eval()
    rng = np.random.default_rng(7)
    keep = SuperResolver(gen, batch_size=48, long_lines=True, keep_sr=True)
    imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * 4)]
    p = keep(imgs)
    pending = keep.exporter.lines(p.sr, p.lines, 2)
    buf, rows = pending.line_canvases
    buf = buf.clone()
    readers = {"beam": plain_reader, "beam_pattern": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4, pattern=pats["plate"])}
    calls = max(1, a.calls // 4)

    def host_window(fn):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls
    fns = {k: (lambda r=r: r.read(buf, rows, 2).result()) for k, r in readers.items()}
    b, f = fns["beam"](), fns["beam_pattern"]()
    assert len(b) == len(f) == 16 and all(r.alternatives for r in b) and all(r.mass == r.mass for r in f)
    res["lines"] = len(rows)
    res["lines_read_as_a_plate"] = sum(bool(r.alternatives) for r in f)
    times = alternate(fns, host_window)
    for k in fns:
        res["reader_%s_ms" % k] = span(times[k], 3)
    res["reader_ranges_overlap"] = overlap(times["beam"], times["beam_pattern"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
