"""Text lines of any width: the host composition `tatt_amd.io.super_resolve_lines_host` (PIL resize and crops, the windows of every line
through a graph session, numpy blend) against `tatt_amd.infer.SuperResolver(long_lines=True)` on the same images and the same generator,
in the same process, alternating the two.  Reports only (one JSON line), asserts nothing but the equality of the results.

    timeout -k 10 300 python tools/bench_lines.py [--lines 16] [--repeats 5] [--warmup 2] [--widths 128,300,600,1200] [--out FILE]

Per width: `--lines` RGB images 40 rows high and that many columns wide (wl = 0.4 x the width at the LR height of 16).  A timed window is
one call over all lines read to the end (PIL images on the host on both paths) and ends in a device synchronise; per repeat every path runs
one window, in an order that rotates with the repeat.  min / median / max over the repeats in milliseconds per call; `disjoint_<width>`
tells whether the device path's range lies wholly below the host path's (only then does it count as faster).  The host path runs the
windows of each line through an `InferenceSession` of that many windows: the model is the same HIP code on both sides, what differs is
everything around it.  TSRN with seeded weights; the device path batches 48 windows across lines."""
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
    ap.add_argument("--lines", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--widths", default="128,300,600,1200")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from PIL import Image
    import tatt_amd
    from tatt_amd import io
    from tatt_amd.build import build
    from tatt_amd.infer import InferenceSession, SuperResolver
    from oracle.fixtures import randomize_state_dict
    from tests.pil_resample_ref import make_image
    build(verbose=False)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    gen.load_state_dict(randomize_state_dict(gen.state_dict()))
    gen = gen.to(dev).eval()
    up = SuperResolver(gen, batch_size=48, long_lines=True)
    sessions = {}

    def run_windows(stack):
        """the windows of one line through a session of their own count (what a caller without the device path would write)"""
        n = stack.shape[0]
        s = sessions.get(n)
        if s is None:
            s = sessions[n] = InferenceSession(gen, batch_size=n)
        return s.run(stack.to(dev))[0].cpu()

    widths = [int(w) for w in a.widths.split(",")]
    rng = np.random.default_rng(7)
    res = {"bench": "lines", "lines": a.lines, "repeats": a.repeats, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    for width in widths:
        imgs = [Image.fromarray(make_image(rng, 40, width, i % 3), "RGB") for i in range(a.lines)]
        fns = {"host": lambda: io.super_resolve_lines_host(imgs, run_windows), "device": lambda: up(imgs).result()}
        want, got = fns["host"](), fns["device"]()
        assert all(np.array_equal(np.asarray(w), np.asarray(g)) for w, g in zip(want, got)), width

        def window(fn):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        names = list(fns)
        for k in names:
            for _ in range(a.warmup):
                window(fns[k])
        times = {k: [] for k in names}
        for r in range(a.repeats):
            for k in names[r % 2:] + names[:r % 2]:
                times[k].append(window(fns[k]))
        span = lambda ts: {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}
        res["windows_%d" % width] = sum(len(io.line_plan(im.size)[1]) for im in imgs)
        for k in names:
            res["%s_ms_%d" % (k, width)] = span(times[k])
        res["disjoint_%d" % width] = bool(max(times["device"]) < min(times["host"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
