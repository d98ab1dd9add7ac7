"""Image export: the host path `tatt_amd.io.export_pil_batch(sr, sizes)` against `tatt_amd.io.DeviceExporter` on the same SR-shaped tensor
(B = 48, 4 x 32 x 128, channels-last strides), in the same process, alternating the two.  Reports only (one JSON line), asserts nothing but
the equality of the results.

    timeout -k 10 300 python tools/bench_export.py [--batches 50] [--repeats 5] [--warmup 5] [--images 480] [--out FILE]

Two geometries: `native` (32 x 128, quantise only) and `resize` (every image to 64 x 256).  A timed window is `batches` exports, each read
to the end (`result()`: PIL images on the host on both paths), and ends in a device synchronise; per repeat every path runs one window, in
an order that rotates with the repeat.  min / median / max over the repeats are reported for each; `disjoint_*` tells whether the device
path's range lies wholly below the host path's (only then does it count as faster).  `host_share_ms_*` is the time until `exporter(...)`
returns (plan, descriptor rows, the three enqueues), the result released unread, timed in windows of its own.  `super_resolver_img_s`:
`SuperResolver` end to end (PIL crops of mixed sizes in, PIL images out, TSRN_TL_TRANS + CRNN prior with seeded weights, batch 48) in
images per second over `--images` crops, min / median / max over the repeats."""
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
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=480, help="crops per SuperResolver window (0: skip that part)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from PIL import Image
    import tatt_amd
    from tatt_amd import io
    from tatt_amd.build import build
    from tatt_amd.infer import SuperResolver
    from oracle.fixtures import randomize_state_dict
    from tests.pil_resample_ref import make_image
    build(verbose=False)
    dev = torch.device("cuda:0")
    x = (torch.rand(48, 4, 32, 128, generator=torch.Generator().manual_seed(48)) * 1.2 - 0.1).to(dev)
    x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)               # the strides the generators return
    ex = io.DeviceExporter(device=dev, rule="floor")
    geoms = {"native": None, "resize": (256, 64)}
    fns, shares = {}, {}
    for g, sizes in geoms.items():
        fns["host_" + g] = lambda sizes=sizes: io.export_pil_batch(x, sizes, "floor")
        fns["device_" + g] = lambda sizes=sizes: ex(x, sizes).result()
        shares[g] = lambda sizes=sizes: ex(x, sizes).release()
        want, got = fns["host_" + g](), fns["device_" + g]()
        assert all(np.array_equal(np.asarray(w), np.asarray(d)) for w, d in zip(want, got)), g

    def window(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def share_window(fn, n):
        torch.cuda.synchronize()
        total = 0.0
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            total += time.perf_counter() - t0
        torch.cuda.synchronize()
        return total / n * 1e3

    names = list(fns)
    for k in names:
        window(fns[k], a.warmup)
    times = {k: [] for k in names}
    share_t = {g: [] for g in geoms}
    for r in range(a.repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(window(fns[k], a.batches))
        for g in geoms:
            share_t[g].append(share_window(shares[g], a.batches))
    rng = lambda ts: {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}
    res = {"bench": "export", "B": 48, "batches": a.batches, "repeats": a.repeats, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    for k in names:
        res[k + "_ms"] = rng(times[k])
    for g in geoms:
        res["disjoint_" + g] = bool(max(times["device_" + g]) < min(times["host_" + g]))
        res["host_share_ms_" + g] = rng(share_t[g])

    if a.images:
        def seeded(m, seed):
            torch.manual_seed(seed)
            m.load_state_dict(randomize_state_dict(m.state_dict(), seed=seed))
            return m.to(dev).eval()
        gen = seeded(tatt_amd.TSRN_TL_TRANS(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32), 1234)
        prior = seeded(tatt_amd.CRNN(32, 1, 37, 256), 5)
        r = np.random.default_rng(41)
        crops = [Image.fromarray(make_image(r, int(r.integers(8, 40)), int(r.integers(24, 160)), i % 3), "RGB") for i in range(a.images)]
        up = SuperResolver(gen, prior=prior, batch_size=48)
        up(crops[:96]).result()                                                 # (captures the sessions)
        rates = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = up(crops).result()
            rates.append(len(out) / (time.perf_counter() - t0))
        res["super_resolver_images"] = a.images
        res["super_resolver_img_s"] = {"min": round(min(rates), 1), "median": round(statistics.median(rates), 1), "max": round(max(rates), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
