"""Polygon text instances (curved text): the host composition `tatt_amd.io.super_resolve_polys_host` (numpy warp per strip, numpy paste
per polygon, PIL resizes, the windows of every polygon through a graph session, numpy blend, PIL up-scale of the scene) against
`tatt_amd.infer.SuperResolver.scene_polys` on the same scene, the same polygons and the same generator, in the same process, alternating
the two.  Reports only (one JSON line), asserts nothing but the equality of the results.

    timeout -k 10 900 python tools/bench_polys.py [--repeats 5] [--calls 4] [--warmup 1] [--cases 720x1280x8x4,720x1280x40x4,..]
                                                  [--feather 2] [--out FILE]

A case is ROWSxCOLUMNSxPOLYGONSxN: a seeded scene of that size and that many seeded polygons of 2 N points: an arc of a ring, 12-48 rows
thick, its centre line 2-10 times as long, bent by up to 25 degrees per strip to either side, turned by up to 30 degrees, every point moved
by up to a twelfth of the thickness, rounded to integers (drawn again until `poly_check` takes it; polygons may overlap).  The default
cases: 8 and 40 polygons in a 720 x 1280 scene, with N = 4 and N = 7.  A timed window is `--calls` calls read to the end (a PIL image on
the host on both paths) and ends in a device synchronise; per repeat every path runs one window, in an order that rotates with the
repeat.  min / median / max over the repeats in milliseconds per call; `disjoint_<case>` tells whether the device path's range lies
wholly below the host path's (only then does it count as faster).  `device_host_share_<case>`: the part of a device call spent on the
host before `result()` is asked for.  `poly_paste_us_<case>`: the tatt_poly_paste_u8 launches of the case alone (all layers), and beside
it `quad_paste_us_<case>`: tatt_warp_u8 mode 1 on the BOUNDING QUADS of the same polygons (t_0, t_{N-1}, b_{N-1}, b_0, each with a line
of its own size; a polygon whose bounding quad `quad_check` refuses is left out of BOTH timings, `paste_timed_<case>` says how many are
in), in the same call: device time per repetition from events around `--calls` x 5 repetitions on prepared buffers, min / median / max
over the repeats, alternating.  `strip_walk_ratio_<case>` = median poly / median quad: what the strip walk costs; `paste_overlap_<case>`
tells whether the two ranges overlap (then the ratio says nothing).  TSRN with seeded weights; the device path batches 48 windows across
polygons.

Every GPU step under its own time limit: run the tool as above, one case per invocation where a case is slow."""
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


def make_polys(rng, hs, ws, n, N):
    from tatt_amd import io
    polys = []
    while len(polys) < n:
        th = int(rng.integers(12, 49))
        length = min(th * rng.uniform(2.0, 10.0), 0.8 * ws)
        bend = math.radians(rng.uniform(-25, 25)) * (N - 1)           # the turn of the centre line over the whole polygon
        if abs(bend) < 1e-3:
            bend = 1e-3
        radius = length / bend                                       # signed: the centre of the ring lies below (+) or above (-) the text
        cx, cy, t = rng.uniform(0, ws), rng.uniform(0, hs), math.radians(rng.uniform(-30, 30))
        top, bot = [], []
        for k in range(N):
            a = bend * (k / (N - 1) - 0.5)                           # the direction of the centre line there
            for side, out in ((-th / 2, top), (th / 2, bot)):         # the centre line's point, moved by `side` along its normal (y down)
                u, v = radius * math.sin(a) - side * math.sin(a), radius * (1 - math.cos(a)) + side * math.cos(a)
                dx, dy = rng.uniform(-th / 12, th / 12, 2)
                out.append((int(round(cx + u * math.cos(t) - v * math.sin(t) + dx)), int(round(cy + u * math.sin(t) + v * math.cos(t) + dy))))
        poly = tuple(top + bot[::-1])
        try:
            io.poly_check((ws, hs), [poly])
            io.line_plan(io.poly_size(poly))
        except ValueError:
            continue
        polys.append(poly)
    return polys


def paste_timers(dev, scene, polys, scale, feather):
    """-> (poly, quad, n): two callables that enqueue the paste launches of the polygons and of their bounding quads on prepared buffers
    (the bytes do not matter to the time), for the n polygons whose bounding quad `quad_check` takes"""
    from tatt_amd import io, ops
    from tatt_amd.polys import POLY_DESC
    from tatt_amd.quads import QUAD_DESC
    keep, quads = [], []
    for p in polys:
        n = len(p) // 2
        q = (p[0], p[n - 1], p[n], p[2 * n - 1])
        try:
            io.quad_check(scene.size, [q])
            io.line_plan(io.quad_size(q))
        except ValueError:
            continue
        keep.append(p)
        quads.append(q)
    if not keep:
        return None, None, 0
    P = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)

    def lines_of(sizes):
        lines = []
        for size in sizes:
            wl, starts = io.line_plan(size)
            lines.append(io.Line(wl, starts, sum(len(ln.starts) for ln in lines)))
        return lines, io.blend_plan(lines, lines[-1].first + len(lines[-1].starts), 16 * scale, 64 * scale, scale)
    lines, (bdesc, _, bbytes) = lines_of([io.poly_size(p) for p in keep])
    pp = io.poly_paste_plan(scene.size, keep, bdesc, bbytes, scale, 16 * scale, feather)
    items, strips = torch.from_numpy(pp.items.copy()), torch.from_numpy(pp.strips.copy())
    items_dev, strips_dev, pout = items.to(dev), strips.to(dev), torch.zeros(pp.nbytes, dtype=torch.uint8, device=dev)
    lines, (bdesc, _, bbytes) = lines_of([io.quad_size(q) for q in quads])
    qp = io.quad_paste_plan(scene.size, quads, bdesc, bbytes, scale, 16 * scale, feather)
    rows = torch.from_numpy(qp.warp.copy())
    rows_dev, qout = rows.to(dev), torch.zeros(qp.nbytes, dtype=torch.uint8, device=dev)

    def poly():
        r = 0
        for c in pp.counts:
            ops.call("tatt_poly_paste_u8", P(pout), pp.canvas_off, P(items_dev, r * POLY_DESC * 4), P(items, r * POLY_DESC * 4), c,
                     P(strips_dev), P(strips), len(pp.strips), P(pout), pp.nbytes, ops.stream())
            r += c

    def quad():
        r = 0
        for c in qp.counts:
            ops.call("tatt_warp_u8", P(qout), qp.canvas_off, P(rows_dev, r * QUAD_DESC * 4), P(rows, r * QUAD_DESC * 4), c, P(qout),
                     qp.nbytes, ops.stream())
            r += c
    return poly, quad, len(keep)


def device_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="720x1280x8x4,720x1280x40x4,720x1280x8x7,720x1280x40x7")
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
        """the windows of one polygon through a session of their own count (what a caller without the device path would write)"""
        n = stack.shape[0]
        s = sessions.get(n)
        if s is None:
            s = sessions[n] = InferenceSession(gen, batch_size=n)
        return s.run(stack.to(dev))[0].cpu()

    rng = np.random.default_rng(7)
    res = {"bench": "polys", "repeats": a.repeats, "calls": a.calls, "feather": a.feather, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    span = lambda ts: {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}
    for case in a.cases.split(","):
        hs, ws, nb, N = (int(v) for v in case.split("x"))
        scene = Image.fromarray(make_image(rng, hs, ws, 0), "RGB")
        polys = make_polys(rng, hs, ws, nb, N)
        host_part = []

        def device():
            t0 = time.perf_counter()
            p = up.scene_polys(scene, polys, a.feather)
            host_part.append(time.perf_counter() - t0)
            return p.result()
        fns = {"host": lambda: io.super_resolve_polys_host(scene, polys, run_windows, feather=a.feather), "device": device}
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
        res["windows_%s" % case] = sum(len(io.line_plan(io.poly_size(p))[1]) for p in polys)
        res["layers_%s" % case] = max(io.poly_layers(polys)) + 1
        for k in names:
            res["%s_ms_%s" % (k, case)] = span(times[k])
        res["device_host_share_%s" % case] = round(statistics.median(host_part) * 1e3 / statistics.median(times["device"]), 3)
        res["disjoint_%s" % case] = bool(max(times["device"]) < min(times["host"]))
        poly, quad, n = paste_timers(dev, scene, polys, 2, a.feather)
        res["paste_timed_%s" % case] = n
        if n:
            us = {"poly": [], "quad": []}
            for r in range(a.repeats):
                for k, fn in (("poly", poly), ("quad", quad))[::1 if r % 2 == 0 else -1]:
                    us[k].append(device_us(fn, 5 * a.calls))
            res["poly_paste_us_%s" % case], res["quad_paste_us_%s" % case] = span(us["poly"]), span(us["quad"])
            res["strip_walk_ratio_%s" % case] = round(statistics.median(us["poly"]) / statistics.median(us["quad"]), 3)
            res["paste_overlap_%s" % case] = bool(min(us["poly"]) <= max(us["quad"]) and min(us["quad"]) <= max(us["poly"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
