"""The five Pillow-resampling entries of csrc/pil_resample.h's two bodies -- tatt_collate_images, tatt_line_windows, tatt_scene_windows
(the window body), tatt_resize_u8, tatt_line_luma (the tile body) -- and the two entries of csrc/warp_pixel.h's pixel functions --
tatt_warp_u8 in both modes, tatt_poly_paste_u8 -- on TWO builds of the library in one process: the tree's
libtatt_hip.so and the one given by --against (the same C ABI, e.g. the parent commit's build), alternating the two.  Both are taken as built
(`python -m tatt_amd.build` first).  Reports only (one JSON line), asserts nothing but that the two libraries write the same bytes.

    timeout -k 10 600 python tools/bench_resamplers.py --against OTHER/libtatt_hip.so [--repeats 9] [--warmup 2] [--window-ms 20] [--out FILE]

Shapes, the defaults of the tools that measure the paths around these entries:
  collate_images  the seeded B = 48 batch of tools/bench_collate.py: 48 HR sources to 32 x 128 and 48 LR sources to 16 x 64, with masks
  line_windows    tools/bench_lines.py: 16 lines of 40 rows at each of 128, 300, 600 and 1200 columns, 16 x 64 windows (four launches)
  scene_windows   tools/bench_scene.py: seeded scenes 720x1280 with 8 and with 40 boxes, 2160x3840 with 40 boxes (three launches)
  resize_u8       the same scenes: the 2 x background and one launch per paste layer, feather 2, from line canvases of seeded bytes
  line_luma       tools/bench_read.py: the line canvases (32 rows, 2 wl columns) of `lines16` and of the 40 boxes of the 720x1280 scene
  warp_rectify    tools/bench_quads.py --cases 720x1280x40: the mode-0 rows of its 40 quads, scene -> crops (one launch)
  warp_paste      the same quads: the mode-1 rows at scale 2, feather 2, rectangles of seeded bytes -> canvas (one launch per layer)
  poly_paste      tools/bench_polys.py --cases 720x1280x40x7: the item and strip rows of its 40 polygons of N = 7, scale 2, feather 2, all layers
The calls go through ctypes with the argument lists the Python layer builds (its `*_plan` functions), the same lists for both libraries.
A timed window is `passes` passes over the entry's launches back to back between two device events, ending in a synchronise; `passes`
is chosen once per entry so that a window lasts about --window-ms (far above the launch overhead) and `launches_<entry>` records
passes x launches.  Per repeat each library runs one window, in an order that rotates with the repeat; `<library>_us_<entry>` is
min / median / max over the repeats in microseconds per pass.  `within_<entry>`: the tree's median is no higher than the other library's
median plus that library's own max - min in this run."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402


def load(path, protos):
    dll = ctypes.CDLL(path)
    for name, args in protos.items():
        fn = getattr(dll, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [t for t, _ in args]
    return dll


class Launch:
    """one call of an entry (src, src size, desc, desc_host, n, out, out size, stream); `out` starts from `init` when results are compared"""

    def __init__(self, dev, name, src, src_size, desc, out, init=None):
        import numpy as np
        self.name, self.src, self.src_size, self.out, self.init = name, src, int(src_size), out, init
        self.host = np.ascontiguousarray(desc, np.int32)
        self.desc = torch.from_numpy(self.host).to(dev)

    def __call__(self, lib):
        from tatt_amd import ops
        rc = getattr(lib, self.name)(ops.P(self.src), self.src_size, ops.P(self.desc), ctypes.c_void_p(self.host.ctypes.data),
                                     len(self.host), ops.P(self.out), self.out.numel(), ops.stream())
        assert rc == 0, (self.name, rc)


class PolyLaunch(Launch):
    """one call of tatt_poly_paste_u8: the items of a layer (`desc`) and the strip table all layers share"""

    def __init__(self, dev, src, src_size, items, strips, out, init=None):
        import numpy as np
        Launch.__init__(self, dev, "tatt_poly_paste_u8", src, src_size, items, out, init)
        self.strips_host = np.ascontiguousarray(strips, np.int32)
        self.strips = torch.from_numpy(self.strips_host).to(dev)

    def __call__(self, lib):
        from tatt_amd import ops
        rc = lib.tatt_poly_paste_u8(ops.P(self.src), self.src_size, ops.P(self.desc), ctypes.c_void_p(self.host.ctypes.data), len(self.host),
                                    ops.P(self.strips), ctypes.c_void_p(self.strips_host.ctypes.data), len(self.strips_host),
                                    ops.P(self.out), self.out.numel(), ops.stream())
        assert rc == 0, (self.name, rc)


def make_cases(dev):
    """-> {entry: [Launch]}"""
    import numpy as np
    from PIL import Image
    from bench_polys import make_polys
    from bench_quads import make_quads
    from bench_scene import make_boxes
    from tatt_amd import io, lines, read, scene
    from tests.pil_resample_ref import make_batch, make_image
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)

    def packed(arrays, offsets, nbytes):
        flat = np.zeros(nbytes, np.uint8)
        for a, o in zip(arrays, offsets):
            flat[o:o + a.size] = a.reshape(-1)
        return up(flat)
    floats = lambda n: torch.empty(n, device=dev)
    cases = {k: [] for k in ("collate_images", "line_windows", "scene_windows", "resize_u8", "line_luma")}

    samples = make_batch(2024, B=48)
    arrays, desc, nbytes, out_floats = io.collate_plan([s[0] for s in samples] + [s[1] for s in samples], [(128, 32)] * 48 + [(64, 16)] * 48)
    cases["collate_images"].append(Launch(dev, "tatt_collate_images", packed(arrays, desc[:, 0], nbytes), nbytes, desc, floats(out_floats)))

    rng = np.random.default_rng(7)
    canvases = [[]]                                                  # per case of tools/bench_read.py: the lines whose canvases a reader is given
    for width in (128, 300, 600, 1200):
        imgs = [Image.fromarray(make_image(rng, 40, width, i % 3), "RGB") for i in range(16)]
        arrays, desc, lns, nbytes, out_floats = lines.lines_plan(imgs)
        cases["line_windows"].append(Launch(dev, "tatt_line_windows", packed(arrays, sorted(set(int(o) for o in desc[:, 0])), nbytes), nbytes,
                                            desc, floats(out_floats)))
        canvases[0] += [lines.Line(ln.wl, ln.starts, 0) for ln in lns[:4]]           # bench_read's lines16: four of each width

    def blend_of(lns):
        first, out = 0, []
        for ln in lns:
            out.append(lines.Line(ln.wl, ln.starts, first))
            first += len(ln.starts)
        return lines.blend_plan(out, first, 32, 128, 2)

    for hs, ws, nb in ((720, 1280, 8), (720, 1280, 40), (2160, 3840, 40)):
        img = Image.fromarray(make_image(rng, hs, ws, 0), "RGB")
        boxes = make_boxes(rng, hs, ws, nb)
        plan = scene.scene_plan(img, boxes)
        src = packed(plan.arrays, plan.offsets, plan.nbytes)
        cases["scene_windows"].append(Launch(dev, "tatt_scene_windows", src, plan.nbytes, plan.desc, floats(plan.out_floats)))
        bdesc, _, bbytes = blend_of(plan.lines)
        paste = scene.paste_plan(img.size, boxes, bdesc, bbytes, 2, 32, 2)
        out = torch.empty(paste.nbytes, dtype=torch.uint8, device=dev)
        init = torch.randint(0, 256, (paste.nbytes,), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(hs + nb))
        cases["resize_u8"].append(Launch(dev, "tatt_resize_u8", src, hs * ws * 3, paste.rows[:1], out, init))
        r = 1
        for c in paste.counts:                                       # (src and out are ONE buffer and only the background launch restores
                                                                     # `init`: the timed passes feather into what the pass before left)
            cases["resize_u8"].append(Launch(dev, "tatt_resize_u8", out, paste.canvas_off, paste.rows[r:r + c], out))
            r += c
        if (hs, nb) == (720, 40):
            canvases.append(plan.lines)
    for lns in canvases:
        bdesc, _, bbytes = blend_of(lns)
        plan = read.read_plan([(int(d[6]), 32, int(d[3]) * int(d[2]), int(d[7])) for d in bdesc], 2)
        src = torch.randint(0, 256, (bbytes,), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(bbytes))
        cases["line_luma"].append(Launch(dev, "tatt_line_luma", src, bbytes, plan.desc, floats(plan.floats)))

    def seeded(n):
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(n))

    def pastes(regions, sizes, plan_of):
        """the paste plan of the regions at scale 2, feather 2, and its buffer: the rectangles and the canvas hold seeded bytes"""
        lns = []
        for size in sizes:
            wl, starts = io.line_plan(size)
            lns.append(lines.Line(wl, starts, sum(len(ln.starts) for ln in lns)))
        bdesc, _, bbytes = lines.blend_plan(lns, lns[-1].first + len(lns[-1].starts), 32, 128, 2)
        plan = plan_of(regions, bdesc, bbytes, 2, 32, 2)
        return plan, torch.empty(plan.nbytes, dtype=torch.uint8, device=dev), seeded(plan.nbytes)

    rng = np.random.default_rng(7)                                   # (the quads and the polygons the two tools draw when given the one case)
    img = Image.fromarray(make_image(rng, 720, 1280, 0), "RGB")
    quads = make_quads(rng, 720, 1280, 40)
    plan = io.quad_plan(img, quads)
    buf = packed(plan.arrays, plan.offsets, plan.nbytes)             # the scene in front, the crops behind it in the same buffer
    cases["warp_rectify"] = [Launch(dev, "tatt_warp_u8", buf, plan.nbytes, plan.warp, buf)]
    paste, out, init = pastes(quads, [io.quad_size(q) for q in quads], lambda *a: io.quad_paste_plan(img.size, *a))
    cases["warp_paste"], r = [], 0
    for c in paste.counts:                                           # (only the first launch restores `init`, as for resize_u8)
        cases["warp_paste"].append(Launch(dev, "tatt_warp_u8", out, paste.canvas_off, paste.warp[r:r + c], out, init if r == 0 else None))
        r += c
    rng = np.random.default_rng(7)
    img = Image.fromarray(make_image(rng, 720, 1280, 0), "RGB")
    polys = make_polys(rng, 720, 1280, 40, 7)
    paste, out, init = pastes(polys, [io.poly_size(p) for p in polys], lambda *a: io.poly_paste_plan(img.size, *a))
    cases["poly_paste"], r = [], 0
    for c in paste.counts:
        cases["poly_paste"].append(PolyLaunch(dev, out, paste.canvas_off, paste.items[r:r + c], paste.strips, out, init if r == 0 else None))
        r += c
    return cases


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", required=True, help="another build of libtatt_hip.so with the same C ABI")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def run(bench, a, make_cases):
    """the two libraries on {entry: [launch]} = make_cases(device) -> the result line, printed and written to a.out.  A launch is called
    with a library and has `out` (the tensor it writes) and `init` (None, or what `out` holds before the compared pass); tools/
    bench_lexicon_core.py measures its entries through this function too."""
    from tatt_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    libs = {"tree": load(LIB_PATH, protos), "against": load(os.path.abspath(a.against), protos)}
    dev = torch.device("cuda:0")
    res = {"bench": bench, "repeats": a.repeats, "window_ms": a.window_ms, "device": torch.cuda.get_device_name(0)}

    def once(lib, launches):
        """one pass from the initial bytes -> every output's bytes"""
        for L in launches:
            if L.init is not None:
                L.out.copy_(L.init)
            elif L.out.dtype == torch.float32:
                L.out.fill_(7.0)
        for L in launches:
            L(lib)
        torch.cuda.synchronize()
        return [L.out.view(torch.uint8).cpu() for L in launches]

    def window(lib, launches, passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            for L in launches:
                L(lib)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / passes

    span = lambda ts: {"min": round(min(ts), 2), "median": round(statistics.median(ts), 2), "max": round(max(ts), 2)}
    for entry, launches in make_cases(dev).items():
        got = {k: once(lib, launches) for k, lib in libs.items()}
        for i, (x, y) in enumerate(zip(got["tree"], got["against"])):
            assert torch.equal(x, y), "%s, launch %d: %d of %d bytes differ" % (entry, i, int((x != y).sum()), x.numel())
        res["bytes_equal_%s" % entry] = sum(x.numel() for x in got["tree"])
        del got
        window(libs["tree"], launches, 3)
        passes = max(10, math.ceil(a.window_ms * 1e3 / window(libs["tree"], launches, 10)))
        res["launches_%s" % entry] = passes * len(launches)
        names = list(libs)
        for k in names:
            for _ in range(a.warmup):
                window(libs[k], launches, passes)
        times = {k: [] for k in names}
        for r in range(a.repeats):
            for k in names[r % 2:] + names[:r % 2]:
                times[k].append(window(libs[k], launches, passes))
        for k in names:
            res["%s_us_%s" % (k, entry)] = span(times[k])
        t, p = res["tree_us_%s" % entry], res["against_us_%s" % entry]
        res["within_%s" % entry] = bool(t["median"] <= p["median"] + (p["max"] - p["min"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    run("resamplers", arguments(), make_cases)
