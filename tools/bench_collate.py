"""Batch collation: the host path `tatt_amd.io.collate_pil_batch(samples, device=dev)` against `tatt_amd.io.DeviceCollator` on the same
decoded images, in the same process, alternating the two.  Reports only (one JSON line), asserts nothing but the equality of the results.

    python tools/bench_collate.py [--batches 50] [--repeats 5] [--warmup 5] [--out FILE]
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python tools/bench_collate.py --census 20 [--lean]   # device path only

The batch is the seeded B = 48 batch of tests/test_collate_device_gpu.py (tests/pil_resample_ref.make_batch, one definition for the test
and the measurement: LR sources 8-39 x 24-159 pixels, HR twice that; smooth, noise and two-level content), decoded beforehand.  A timed
window is `batches` calls and ends in a device synchronise; per repeat every path runs one window, in an order that rotates with the
repeat.  Three paths: `host` (collate_pil_batch: always all four stacks), `device_yuv` (DeviceCollator(want_yuv=True): the same four
stacks, like for like) and `device_lean` (want_yuv=False: the two stacks the TATT recipes read -- less work, not only faster work).
min / median / max over the repeats are reported for each; `disjoint_*` tells whether a device path's range lies wholly below the host
path's (only then does it count as faster).  `host_share_ms_*` is the host side of a device call alone -- plan, label encoding and the
slot fill into an ordinary buffer, nothing enqueued -- timed in windows of its own."""
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
    ap.add_argument("--census", type=int, default=0, help="run only N device-path calls (for a profiler run) and exit")
    ap.add_argument("--lean", action="store_true", help="with --census: want_yuv=False")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from tatt_amd import io
    from tatt_amd.build import build
    from tests.pil_resample_ref import make_batch
    build(verbose=False)
    dev = torch.device("cuda:0")
    samples = make_batch(2024, B=48)
    kw = dict(imgH=32, imgW=128, down_sample_scale=2, mask=True, device=dev)
    cols = {"device_yuv": io.DeviceCollator(want_yuv=True, **kw), "device_lean": io.DeviceCollator(want_yuv=False, **kw)}
    if a.census:
        col = cols["device_lean" if a.lean else "device_yuv"]
        for _ in range(a.census):
            col(samples)
        torch.cuda.synchronize()
        print(json.dumps({"census_calls": a.census, "want_yuv": not a.lean}))
        return
    fns = {"host": lambda: io.collate_pil_batch(samples, **kw)}
    fns.update({k: (lambda c=c: c(samples)) for k, c in cols.items()})
    want, full, lean = fns["host"](), fns["device_yuv"](), fns["device_lean"]()
    torch.cuda.synchronize()
    assert all(torch.equal(want[m], full[m]) for m in (0, 2, 3, 4, 6)) and all(torch.equal(want[m], lean[m]) for m in (0, 2, 6))

    def window(fn, n, sync=True):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        if sync:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def host_share(col):
        scratch = np.empty(1 << 24, np.uint8)

        def fn():
            (arrays, desc, _, _), labels, _ = col.plan(samples)
            vecs, _, _ = io.collate_labels(labels, col.alphabet)
            io.collate_fill(scratch, arrays, desc, vecs.numpy())
        return fn

    names = list(fns)
    for k in names:
        window(fns[k], a.warmup)
    times = {k: [] for k in names}
    shares = {k: [] for k in cols}
    for r in range(a.repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            times[k].append(window(fns[k], a.batches))
        for k, c in cols.items():
            shares[k].append(window(host_share(c), a.batches, sync=False))
    rng = lambda ts: {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}
    res = {"bench": "collate", "B": 48, "batches": a.batches, "repeats": a.repeats, "cpu_threads": torch.get_num_threads(),
           "device": torch.cuda.get_device_name(0)}
    for k in names:
        res[k + "_ms"] = rng(times[k])
    for k in cols:
        res["disjoint_" + k] = bool(max(times[k]) < min(times["host"]))
        res["host_share_ms_" + k] = rng(shares[k])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
