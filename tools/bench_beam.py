"""The CTC prefix beam search beside the greedy decoding (csrc/ctcbeam.hip, csrc/read.hip): the two launches alone on given logits, and
`tatt_amd.read.LineReader` under both decodings, in one process, alternating.  Reports only (one JSON line); asserts nothing but that the
beam's best string was decoded for every line.

    timeout -k 10 600 python tools/bench_beam.py [--repeats 5] [--calls 20] [--warmup 1] [--out FILE]

Launches alone, on seeded logits (randn * 3, C = 37) at (T, n) = (26, 48) and (256, 16): `greedy`, `beam8`, `beam16` (nbest 4), and
`forward`: the chunk's CRNN forward (`LineReader.forward` on an (n, 1, 32, 4 (T - 1)) input) -- device time from events around `--calls`
launches, microseconds per launch; per repeat every candidate runs one such window, in an order that rotates with the repeat; min / median
/ max over the repeats.
The reader: the 16 lines of tools/bench_read.py's `lines16` case (four each of 128, 300, 600 and 1200 columns at 40 rows, blended once),
`LineReader.read(...).result()` with decode="greedy" and decode="beam" (beam 8, nbest 4), host time of a window of `--calls // 4` calls that
ends in a device synchronise, milliseconds per call, same alternation; `reader_ranges_overlap`: whether the two ranges overlap.
TSRN and CRNN with seeded weights; batch_size 48."""
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
    res = {"bench": "beam", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
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
    reader = read.LineReader(crnn, batch_size=48)
    for T, n in ((26, 48), (256, 16)):
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        img = torch.rand(n, 1, 32, 4 * (T - 1), generator=torch.Generator().manual_seed(n)).to(dev)
        assert reader.forward(img).shape == (T, n, 37)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        greedy_rec = torch.empty(n, 3 * T + 2, dtype=torch.int32, device=dev)
        beam_rec = torch.empty(n, read.beam_record_words(T, 4), dtype=torch.int32, device=dev)
        fns = {"greedy": lambda: read.ctc_greedy_read(x, index, greedy_rec, T),
               "beam8": lambda: read.ctc_beam_read(x, index, beam_rec, T, 8, 4),
               "beam16": lambda: read.ctc_beam_read(x, index, beam_rec, T, 16, 4),
               "forward": lambda: reader.forward(img)}
        times = alternate(fns, device_window)
        for k in fns:
            res["%s_us_T%d_n%d" % (k, T, n)] = span(times[k])
        got = read.parse_beam_records(beam_rec.cpu(), T, 4)
        assert all(g.flag == 0 and g.entries for g in got)

    # ---- the reader under both decodings ----
    rng = np.random.default_rng(7)
    keep = SuperResolver(gen, batch_size=48, long_lines=True, keep_sr=True)
    imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * 4)]
    p = keep(imgs)
    pending = keep.exporter.lines(p.sr, p.lines, 2)
    buf, rows = pending.line_canvases
    buf = buf.clone()
    readers = {"greedy": reader, "beam": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4)}
    calls = max(1, a.calls // 4)

    def host_window(fn):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls
    fns = {k: (lambda r=r: r.read(buf, rows, 2).result()) for k, r in readers.items()}
    g, b = fns["greedy"](), fns["beam"]()
    assert len(g) == len(b) == 16 and all(r.alternatives for r in b)
    res["lines"] = len(rows)
    res["beam_best_differs_from_greedy"] = sum(x.text != y.text for x, y in zip(g, b))
    times = alternate(fns, host_window)
    for k in fns:
        res["reader_%s_ms" % k] = span(times[k], 3)
    res["reader_ranges_overlap"] = bool(min(times["beam"]) <= max(times["greedy"]) and min(times["greedy"]) <= max(times["beam"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
