"""The MORAN recogniser's two fused launches against their comparators, in the same process, alternating.  Reports only (one JSON line).

    timeout -k 10 600 python tools/bench_moran.py [--repeats 5] [--calls 5] [--warmup 1] [--batches 1,48] [--out FILE]

  decode      one launch (`moran.attn_decode` -> tatt_moran_decode) against the step-by-step route (`moran.decode_eager`: about a dozen
              launches per step on the shared operators), greedy, L = 20, T = 25, 37 classes, randn features, seeded weights
  rectify     `moran.morn_rectify` (tatt_morn_rectify, both passes' tails) against the same tail written with torch's device operators
              (relu, max_pool2d, grid_sample, cat), on the same seeded offsets maps and images
  read        `MORAN.read` end to end (rectifier, encoder, L2R decoder) on seeded images, and its launch census
A timed window is `--calls` calls and ends in a device synchronise; per repeat every route runs one window, in an order that rotates
with the repeat; min / median / max over the repeats in milliseconds per call.  `disjoint_<what>_b<B>`: whether the fused launch's
range lies wholly below its comparator's -- the only sense in which it counts as faster.  `census_*`: library launches of one call
(torch's own kernels are not counted).  One process under the one outer `timeout -k 10`, as tools/bench_aster.py; like that tool it
borrows a helper from tests/ (tests/moran_ref.py: seeded weights, features and images)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def torch_tail(o, x, grid, acc=None):
    """the rectifier's tail as the reference writes it, on torch's device operators: o (B, 1, h, w), x (B, C, H, W), grid (B, H, W, 2)"""
    F = torch.nn.functional
    pool = F.max_pool2d(F.relu(o), 2, 1) - F.max_pool2d(F.relu(-o), 2, 1)
    g = F.grid_sample(pool, grid, align_corners=False).permute(0, 2, 3, 1).contiguous()
    acc = g if acc is None else acc + g
    return F.grid_sample(x, torch.cat([grid[..., :1], grid[..., 1:] + acc], 3), align_corners=False), acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="1,48")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import tatt_amd
    from tatt_amd import moran, ops
    from tatt_amd._lib import LIB_PATH
    import moran_ref as R
    if not os.path.exists(LIB_PATH):
        from tatt_amd.build import build
        build(verbose=False)
    dev = torch.device("cuda:0")
    model = R.e2e_model(tatt_amd.MORAN).to(dev).eval()
    att = model.ASRN.attentionL2R
    operands = moran.decoder_operands(att)
    L, T = moran.MAX_ITER, 25
    res = {"bench": "moran", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0), "steps": L, "classes": att.num_classes}

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

    def census(fn):
        n, real = [0], ops.call

        def counted(name, *args):
            n[0] += 1
            return real(name, *args)
        ops.call = counted
        before = moran.LAUNCHES["one_launch"]
        try:
            fn()
        finally:
            ops.call = real
        return n[0] + moran.LAUNCHES["one_launch"] - before         # (tatt_moran_decode is called past ops.call: it may return 1)

    def report(tag, fns, fused, other):
        times = alternate(fns)
        for k in fns:
            res["%s_%s_ms" % (tag, k)] = span(times[k])
        res["disjoint_" + tag] = bool(max(times[fused]) < min(times[other]))

    gx, gy = R.regular_grid(32, 100, np.float32)
    with torch.no_grad():
        for B in [int(v) for v in a.batches.split(",")]:
            x = R.features(B, T, 3).to(dev)
            fns = {"eager": lambda: moran.decode_eager(att, x, 1, steps=L), "one_launch": lambda: moran.attn_decode(att, x, 1, steps=L, operands=operands)}
            ids_e, ids_o = fns["eager"]()[0], fns["one_launch"]()[0]
            res["ids_equal_decode_b%d" % B] = "%d/%d" % (int((ids_e == ids_o).all(1).sum()), B)
            res["census_decode_b%d" % B] = {k: census(f) for k, f in fns.items()}
            report("decode_b%d" % B, fns, "one_launch", "eager")

            g = torch.Generator().manual_seed(5)
            img = R.images(B, seed=6).to(dev)
            o1 = (torch.rand(B, 4, 12, generator=g) * 0.8 - 0.4).to(dev)
            o2 = (torch.rand(B, 4, 12, generator=g) * 0.8 - 0.4).to(dev)
            grid = torch.stack([torch.from_numpy(gx)[None, :].expand(32, 100), torch.from_numpy(gy)[:, None].expand(32, 100)], 2)
            grid = grid[None].expand(B, 32, 100, 2).contiguous().to(dev)

            def fused():
                _, acc = moran.morn_rectify(o1, img, (32, 100))
                return moran.morn_rectify(o2, img, (32, 100), acc)[0]

            def chain():
                _, acc = torch_tail(o1[:, None], img, grid)
                return torch_tail(o2[:, None], img, grid, acc)[0]
            res["rectify_max_diff_b%d" % B] = float((fused().permute(0, 3, 1, 2) - chain()).abs().max())
            report("rectify_b%d" % B, {"torch_chain": chain, "one_launch": fused}, "one_launch", "torch_chain")

            times = alternate({"read": lambda: model.read(img)})
            res["read_ms_b%d" % B] = span(times["read"])
            res["read_images_per_s_b%d" % B] = round(B * 1e3 / statistics.median(times["read"]), 1)
            res["census_read_b%d" % B] = census(lambda: model.read(img))
    tatt_amd.sync_check()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
