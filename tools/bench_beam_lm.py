"""The beam search with and without the fused character n-gram model (csrc/ctcbeam.hip): the launches alone on given logits, and
`tatt_amd.read.LineReader(decode="beam")` with and without lm=, in one process, alternating.  Reports only (one JSON line); asserts
nothing but that every line was decoded.

    timeout -k 10 600 python tools/bench_beam_lm.py [--repeats 5] [--calls 50] [--warmup 1] [--out FILE]

Expectation, stated before any measurement: the fusion adds BM loads from a table that lives in L2 and a few float64 additions to a step
of roughly 7 us, so it should be a small fraction of the plain launch.  The tool prints ranges and whether they overlap; it promises no
ratio.
Launches alone, on seeded logits (randn * 3, C = 37) at (T, n) = (26, 48) and (256, 16), beam 8, nbest 4: `plain` (tatt_ctc_beam_read)
and `lm1`, `lm2`, `lm3` (tatt_ctc_beam_lm_read with a seeded table of that order) -- device time from events around `--calls` launches,
microseconds per launch; per repeat every candidate runs one such window, in an order that rotates with the repeat; min / median / max
over the repeats; `lmK_overlaps_plain`: whether the two ranges overlap.
The reader: the 16 lines of tools/bench_read.py's `lines16` case, `LineReader.read(...).result()` with decode="beam" (beam 8, nbest 4)
without and with lm= (order 3), host time of a window of `--calls // 4` calls that ends in a device synchronise, milliseconds per call,
same alternation.  TSRN and CRNN with seeded weights; batch_size 48.  The library is the one the build left in the tree (python -m tatt_amd.build)."""
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
    res = {"bench": "beam_lm", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
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

    def model(order):
        g = torch.Generator().manual_seed(order)
        return read.CharLM(torch.log_softmax(torch.randn((37,) * order, generator=g, dtype=torch.float64) * 2, -1).numpy())

    # ---- the launches alone ----
    models = {k: model(k) for k in (1, 2, 3)}
    tables = {k: torch.from_numpy(m.increments(.5, 0.0)).to(dev) for k, m in models.items()}
    for T, n in ((26, 48), (256, 16)):
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        plain_rec = torch.empty(n, read.beam_record_words(T, 4), dtype=torch.int32, device=dev)
        lm_rec = torch.empty(n, read.beam_lm_record_words(T, 4), dtype=torch.int32, device=dev)
        fns = {"plain": lambda: read.ctc_beam_read(x, index, plain_rec, T, 8, 4)}
        for k in (1, 2, 3):
            fns["lm%d" % k] = lambda k=k: read.ctc_beam_lm_read(x, tables[k], k, index, lm_rec, T, 8, 4)
        times = alternate(fns, device_window)
        for k in fns:
            res["%s_us_T%d_n%d" % (k, T, n)] = span(times[k])
            if k != "plain":
                res["%s_overlaps_plain_T%d_n%d" % (k, T, n)] = overlap(times[k], times["plain"])
        assert all(g.flag == 0 and g.entries for g in read.parse_beam_records(plain_rec.cpu(), T, 4))
        assert all(g.flag == 0 and g.entries for g in read.parse_beam_lm_records(lm_rec.cpu(), T, 4))

    # ---- the reader without and with the model ----
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    gen.load_state_dict(randomize_state_dict(gen.state_dict()))
    gen = gen.to(dev).eval()
    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    crnn.load_state_dict(randomize_state_dict(crnn.state_dict(), seed=11))
    crnn = crnn.to(dev).eval()
    rng = np.random.default_rng(7)
    keep = SuperResolver(gen, batch_size=48, long_lines=True, keep_sr=True)
    imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * 4)]
    p = keep(imgs)
    pending = keep.exporter.lines(p.sr, p.lines, 2)
    buf, rows = pending.line_canvases
    buf = buf.clone()
    readers = {"beam": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4),
               "beam_lm": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4, lm=models[3])}
    calls = max(1, a.calls // 4)

    def host_window(fn):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls
    fns = {k: (lambda r=r: r.read(buf, rows, 2).result()) for k, r in readers.items()}
    b, f = fns["beam"](), fns["beam_lm"]()
    assert len(b) == len(f) == 16 and all(r.alternatives for r in b) and all(r.alternatives for r in f)
    res["lines"] = len(rows)
    res["fused_best_differs_from_beam"] = sum(x.text != y.text for x, y in zip(b, f))
    times = alternate(fns, host_window)
    for k in fns:
        res["reader_%s_ms" % k] = span(times[k], 3)
    res["reader_ranges_overlap"] = overlap(times["beam"], times["beam_lm"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
