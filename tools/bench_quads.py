"""Quadrilateral text boxes: the host composition `tatt_amd.io.super_resolve_quads_host` (numpy warp per quad, PIL resizes, the windows
of every quad through a graph session, numpy blend, PIL up-scale of the scene) against `tatt_amd.infer.SuperResolver.scene_quads` on the
same scene, the same quads and the same generator, in the same process, alternating the two.  Reports only (one JSON line), asserts
nothing but the equality of the results.

    timeout -k 10 600 python tools/bench_quads.py [--repeats 5] [--calls 4] [--warmup 1] [--cases 720x1280x8,720x1280x40,2160x3840x40]
                                                  [--feather 2] [--out FILE]

A case is ROWSxCOLUMNSxQUADS: a seeded scene of that size and that many seeded quads: a rectangle 12-60 rows high and 1-12 times as wide,
turned by up to 30 degrees about its centre, every corner moved by up to an eighth of the height, rounded to integers (drawn again until
`quad_check` takes it; quads may overlap).  A timed window is `--calls` calls read to the end (a PIL image on the host on both paths) and
ends in a device synchronise; per repeat every path runs one window, in an order that rotates with the repeat.  min / median / max over
the repeats in milliseconds per call; `disjoint_<case>` tells whether the device path's range lies wholly below the host path's (only
then does it count as faster).  `device_host_share_<case>`: the part of a device call spent on the host before `result()` is asked for.
`warp_rectify_us_<case>` / `warp_paste_us_<case>`: tatt_warp_u8 alone, the rectify launch of the case and its paste launches (all
layers), device time per call from events around `--calls` x 5 repetitions of the launches on prepared buffers.  TSRN with seeded weights;
the device path batches 48 windows across quads.

Every GPU step under its own time limit: run the tool as above, one case per invocation where a case is slow (`--cases 2160x3840x40`)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def make_quads(rng, hs, ws, n):
    from tatt_amd import io
    quads = []
    while len(quads) < n:
        bh = int(rng.integers(12, 61))
        bw = min(bh * rng.uniform(1.0, 12.0), 0.8 * ws)
        cx, cy, t = rng.uniform(0, ws), rng.uniform(0, hs), math.radians(rng.uniform(-30, 30))
        quad = []
        for u, v in ((-bw / 2, -bh / 2), (bw / 2, -bh / 2), (bw / 2, bh / 2), (-bw / 2, bh / 2)):
            dx, dy = rng.uniform(-bh / 8, bh / 8, 2)
            quad.append((int(round(cx + u * math.cos(t) - v * math.sin(t) + dx)), int(round(cy + u * math.sin(t) + v * math.cos(t) + dy))))
        try:
            io.quad_check((ws, hs), [quad])
            io.line_plan(io.quad_size(quad))
        except ValueError:
            continue
        quads.append(tuple(quad))
    return quads


def time_warps(dev, scene, quads, scale, feather, reps):
    """device time per call of the rectify launch and of the paste launches, on prepared buffers (the rectangles hold what the rectify
    left: the bytes do not matter to the time)"""
    import numpy as np
    from tatt_amd import io, ops
    from tatt_amd.quads import QUAD_DESC
    plan = io.quad_plan(scene, quads)
    o_warp, _, _, pix, used, total = io.quad_fill(None, plan)
    flat = np.zeros(total, np.uint8)
    io.quad_fill(flat[:used], plan)
    buf, host = torch.from_numpy(flat).to(dev), torch.from_numpy(flat)
    lines = plan.lines
    bdesc, _, bbytes = io.blend_plan(lines, lines[-1].first + len(lines[-1].starts), 16 * scale, 64 * scale, scale)
    paste = io.quad_paste_plan(scene.size, quads, bdesc, bbytes, scale, 16 * scale, feather)
    rows = torch.from_numpy(paste.warp.copy())
    rows_dev, out = rows.to(dev), torch.zeros(paste.nbytes, dtype=torch.uint8, device=dev)
    P = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)

    def rectify():
        ops.call("tatt_warp_u8", P(buf, pix), plan.nbytes, P(buf, o_warp), P(host, o_warp), len(plan.warp), P(buf, pix), plan.nbytes,
                 ops.stream())

    def pastes():
        r = 0
        for c in paste.counts:
            ops.call("tatt_warp_u8", P(out), paste.canvas_off, P(rows_dev, r * QUAD_DESC * 4), P(rows, r * QUAD_DESC * 4), c, P(out),
                     paste.nbytes, ops.stream())
            r += c
    res = []
    for fn in (rectify, pastes):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        res.append(round(a.elapsed_time(b) * 1e3 / reps, 2))
    return res


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
        """the windows of one quad through a session of their own count (what a caller without the device path would write)"""
        n = stack.shape[0]
        s = sessions.get(n)
        if s is None:
            s = sessions[n] = InferenceSession(gen, batch_size=n)
        return s.run(stack.to(dev))[0].cpu()

    rng = np.random.default_rng(7)
    res = {"bench": "quads", "repeats": a.repeats, "calls": a.calls, "feather": a.feather, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    for case in a.cases.split(","):
        hs, ws, nb = (int(v) for v in case.split("x"))
        scene = Image.fromarray(make_image(rng, hs, ws, 0), "RGB")
        quads = make_quads(rng, hs, ws, nb)
        host_part = []

        def device():
            t0 = time.perf_counter()
            p = up.scene_quads(scene, quads, a.feather)
            host_part.append(time.perf_counter() - t0)
            return p.result()
        fns = {"host": lambda: io.super_resolve_quads_host(scene, quads, run_windows, feather=a.feather), "device": device}
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
        res["windows_%s" % case] = sum(len(io.line_plan(io.quad_size(q))[1]) for q in quads)
        res["layers_%s" % case] = max(io.quad_layers(quads)) + 1
        for k in names:
            res["%s_ms_%s" % (k, case)] = span(times[k])
        res["device_host_share_%s" % case] = round(statistics.median(host_part) * 1e3 / statistics.median(times["device"]), 3)
        res["disjoint_%s" % case] = bool(max(times["device"]) < min(times["host"]))
        res["warp_rectify_us_%s" % case], res["warp_paste_us_%s" % case] = time_warps(dev, scene, quads, 2, a.feather, 5 * a.calls)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
