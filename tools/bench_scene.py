"""Scene images: the host composition `tatt_amd.io.super_resolve_scene_host` (PIL crop, resize and paste per box, the windows of every
box through a graph session, numpy blend, PIL up-scale of the scene) against `tatt_amd.infer.SuperResolver.scene` on the same scene, the
same boxes and the same generator, in the same process, alternating the two.  Reports only (one JSON line), asserts nothing but the
equality of the results.

    timeout -k 10 600 python tools/bench_scene.py [--repeats 5] [--calls 4] [--warmup 1] [--cases 720x1280x8,720x1280x40,2160x3840x40]
                                                  [--feather 2] [--out FILE]

A case is ROWSxCOLUMNSxBOXES: a seeded scene of that size and that many seeded boxes 12-60 rows high and 1-12 times as wide (so that
single windows and long lines both occur; boxes may overlap).  A timed window is `--calls` calls read to the end (a PIL image on the host
on both paths) and ends in a device synchronise; per repeat every path runs one window, in an order that rotates with the repeat.
min / median / max over the repeats in milliseconds per call; `disjoint_<case>` tells whether the device path's range lies wholly
below the host path's (only then does it count as faster).  `device_host_share_<case>`: the part of a device call spent on the host
before `result()` is asked for (planning, packing the pinned slot, enqueueing), a host clock around the call alone over the window's
time per call.  The host path runs the windows of each box through an `InferenceSession` of that many windows: the model is the same
HIP code on both sides, what differs is everything around it.  TSRN with seeded weights; the device path batches 48 windows across boxes.

Every GPU step under its own time limit: run the tool as above, one case per invocation where a case is slow (`--cases 2160x3840x40`)."""
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
    ap.add_argument("--cases", default="720x1280x8,720x1280x40,2160x3840x40")
    ap.add_argument("--feather", type=int, default=2)
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
    up = SuperResolver(gen, batch_size=48)
    sessions = {}

    def run_windows(stack):
        """the windows of one box through a session of their own count (what a caller without the device path would write)"""
        n = stack.shape[0]
        s = sessions.get(n)
        if s is None:
            s = sessions[n] = InferenceSession(gen, batch_size=n)
        return s.run(stack.to(dev))[0].cpu()

    rng = np.random.default_rng(7)
    res = {"bench": "scene", "repeats": a.repeats, "calls": a.calls, "feather": a.feather, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    for case in a.cases.split(","):
        hs, ws, nb = (int(v) for v in case.split("x"))
        scene = Image.fromarray(make_image(rng, hs, ws, 0), "RGB")
        boxes = make_boxes(rng, hs, ws, nb)
        host_part = []

        def device():
            t0 = time.perf_counter()
            p = up.scene(scene, boxes, a.feather)
            host_part.append(time.perf_counter() - t0)
            return p.result()
        fns = {"host": lambda: io.super_resolve_scene_host(scene, boxes, run_windows, feather=a.feather), "device": device}
        want, got = fns["host"](), fns["device"]()
        assert np.array_equal(np.asarray(want), np.asarray(got)), case

        def window(fn):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        names = list(fns)
        for k in names:
            for _ in range(a.warmup):
                window(fns[k])
        times = {k: [] for k in names}
        del host_part[:]
        for r in range(a.repeats):
            for k in names[r % 2:] + names[:r % 2]:
                times[k].append(window(fns[k]))
        span = lambda ts: {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}
        res["windows_%s" % case] = sum(len(io.line_plan((x1 - x0, y1 - y0))[1]) for x0, y0, x1, y1 in boxes)
        res["layers_%s" % case] = max(io.scene_layers(boxes)) + 1
        for k in names:
            res["%s_ms_%s" % (k, case)] = span(times[k])
        res["device_host_share_%s" % case] = round(statistics.median(host_part) * 1e3 / statistics.median(times["device"]), 3)
        res["disjoint_%s" % case] = bool(max(times["device"]) < min(times["host"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
