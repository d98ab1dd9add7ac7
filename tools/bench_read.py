"""Reading lines at their own width: the host composition `tatt_amd.read.read_lines_host` (PIL resize and numpy luma per line, the eager
CRNN module per line at B = 1, the decoding on the host) against `tatt_amd.read.LineReader` on the same blended lines and the same
recogniser, in the same process, alternating the two.  Reports only (one JSON line), asserts nothing but the equality of the strings'
lengths and widths (the two recognisers differ by the BatchNorm fold, so a string may differ at a near-tie; `text_differences_<case>`
counts them).

    timeout -k 10 600 python tools/bench_read.py [--repeats 5] [--calls 4] [--warmup 1] [--cases lines16,720x1280x8,720x1280x40] [--out FILE]

Cases: `lines16`: 16 text lines, four each of 128, 300, 600 and 1200 columns at 40 rows (`SuperResolver(long_lines=True)`); ROWSxCOLUMNSxBOXES:
a seeded scene with that many seeded boxes (`SuperResolver.scene`, the boxes of tools/bench_scene.py).  Per case the lines are blended once
by the device path; the host path reads them from host memory (its download is not timed), the device path where they lie in device memory.
A timed window is `--calls` reads to the end (the `Reading` records on the host on both paths) and ends in a device synchronise; per repeat
every path runs one window, in an order that rotates with the repeat; min / median / max over the repeats in milliseconds per call;
`disjoint_<case>`: whether the device path's range lies wholly below the host path's.  Further, per case:
  census_<case>            launches of one device read: tatt_line_luma, CRNN forwards (bucket chunks), tatt_ctc_greedy_read (+ one copy back)
  device_host_share_<case> the part of a device read spent on the host before `result()` is asked for
  luma_us_<case> / decode_us_<case>   the two new kernels alone (decode: all chunks), device time from events around repetitions on
                           prepared buffers
  e2e_plain_ms_<case> / e2e_reader_ms_<case>   the whole SuperResolver call without and with `reader=`, same windows
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


def make_boxes(rng, hs, ws, n):
    """the boxes of tools/bench_scene.py: 12-60 rows high and 1-12 times as wide (single windows and long lines both occur)"""
    boxes = []
    while len(boxes) < n:
        bh = int(rng.integers(12, 61))
        bw = min(int(bh * rng.uniform(1.0, 12.0)), ws)
        x0, y0 = int(rng.integers(0, ws - bw + 1)), int(rng.integers(0, hs - bh + 1))
        boxes.append((x0, y0, x0 + bw, y0 + bh))
    return boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="lines16,720x1280x8,720x1280x40")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from PIL import Image
    import tatt_amd
    from tatt_amd import ops, read
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
    rng = np.random.default_rng(7)
    res = {"bench": "read", "repeats": a.repeats, "calls": a.calls, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}

    def eager(x):
        with torch.no_grad():
            return crnn(x.to(dev)).cpu()

    def window(fn):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    def alternate(fns):
        names = list(fns)
        for k in names:
            for _ in range(a.warmup):
                window(fns[k])
        times = {k: [] for k in names}
        for r in range(a.repeats):
            for k in names[r % 2:] + names[:r % 2]:
                times[k].append(window(fns[k]))
        return times
    span = lambda ts: {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}

    for case in a.cases.split(","):
        long = case.startswith("lines")
        plain = SuperResolver(gen, batch_size=48, long_lines=long)
        up = SuperResolver(gen, batch_size=48, long_lines=long, reader=crnn)
        keep = SuperResolver(gen, batch_size=48, long_lines=long, keep_sr=True)
        if case.startswith("lines"):
            n = int(case[5:])
            imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * (n // 4))]
            e2e = {"plain": lambda: plain(imgs).result(), "reader": lambda: up(imgs).result()}
            p = keep(imgs)
        else:
            hs, ws, nb = (int(v) for v in case.split("x"))
            scene = Image.fromarray(make_image(rng, hs, ws, 0), "RGB")
            boxes = make_boxes(rng, hs, ws, nb)
            e2e = {"plain": lambda: plain.scene(scene, boxes).result(), "reader": lambda: up.scene(scene, boxes).texts()}
            p = keep.scene(scene, boxes)
        # the blended lines, once: in device memory (a copy the exporter's later calls leave alone) and in host memory
        pending = keep.exporter.lines(p.sr, p.lines, 2)
        buf, rows = pending.line_canvases
        buf = buf.clone()
        lines_u8 = pending.arrays()
        reader = up.reader
        host_part = []

        def device():
            t0 = time.perf_counter()
            p = reader.read(buf, rows, 2)
            host_part.append(time.perf_counter() - t0)
            return p.result()
        fns = {"host": lambda: read.read_lines_host(lines_u8, eager, scale=2), "device": device}
        want, got = fns["host"](), fns["device"]()
        assert [(r.rw, r.squeezed) for r in want] == [(r.rw, r.squeezed) for r in got], case
        res["lines_%s" % case] = len(rows)
        res["buckets_%s" % case] = len(set(r.rw for r in got))
        res["text_differences_%s" % case] = sum(w.text != g.text for w, g in zip(want, got))
        # census of one device read
        census, real_call, real_fwd = {"tatt_line_luma": 0, "forwards": 0, "tatt_ctc_greedy_read": 0}, ops.call, reader.forward
        line_luma = read.line_luma

        def counted_luma(*args):
            census["tatt_line_luma"] += 1
            return line_luma(*args)

        def counted_call(name, *args):
            if name in census:
                census[name] += 1
            return real_call(name, *args)

        def counted_fwd(x):
            census["forwards"] += 1
            return real_fwd(x)
        ops.call, reader.forward, read.line_luma = counted_call, counted_fwd, counted_luma
        try:
            reader.read(buf, rows, 2).result()
        finally:
            ops.call, read.line_luma = real_call, line_luma
            del reader.forward
        res["census_%s" % case] = census
        del host_part[:]
        times = alternate(fns)
        for k in fns:
            res["%s_ms_%s" % (k, case)] = span(times[k])
        res["device_host_share_%s" % case] = round(statistics.median(host_part) * 1e3 / statistics.median(times["device"]), 3)
        res["disjoint_%s" % case] = bool(max(times["device"]) < min(times["host"]))
        # the two new kernels alone
        plan = read.read_plan(rows, 2)
        desc_dev, luma = torch.from_numpy(plan.desc).to(dev), torch.empty(plan.floats, device=dev)
        kept = reader.read(buf, rows, 2, keep_logits=True)
        kept.result()
        cap = max(plan.rws) // 4 + 1
        record = torch.empty(len(rows), 3 * cap + 2, dtype=torch.int32, device=dev)
        index = [torch.tensor(idx, dtype=torch.int32).to(dev) for idx, _ in kept.logits]

        def decode():
            for ix, (_, lg) in zip(index, kept.logits):
                read.ctc_greedy_read(lg, ix, record, cap)
        reps = 5 * a.calls
        for name, fn in (("luma", lambda: read.line_luma(buf, desc_dev, plan.desc, luma)), ("decode", decode)):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            res["%s_us_%s" % (name, case)] = round(e0.elapsed_time(e1) * 1e3 / reps, 2)
        times = alternate(e2e)
        for k in e2e:
            res["e2e_%s_ms_%s" % (k, case)] = span(times[k])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
