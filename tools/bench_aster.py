"""The ASTER attention decoder: the step-by-step route (`aster.decode_eager`: about a dozen launches per step on the shared operators, torch
for the beam's bookkeeping, one launch for its backtracking; nothing of it runs on the host) against the one launch (`aster.attn_decode` -> tatt_attn_decode), beam and
greedy, at B = 1 and B = 48, in the same process, alternating the two.  Reports only (one JSON line).

    timeout -k 10 600 python tools/bench_aster.py [--repeats 5] [--calls 3] [--warmup 1] [--batches 1,48] [--out FILE]

A timed window is `--calls` decodings of the same encoder features (randn (B, 25, 512), seeded decoder weights with fc.weight x 30, 97
classes, 100 steps) and ends in a device synchronise; per repeat every route runs one window, in an order that rotates with the
repeat; min / median / max over the repeats in milliseconds per decoding.  `disjoint_<mode>_b<B>`: whether the one launch's range lies
wholly below the step-by-step route's -- the only sense in which it counts as faster.  Further:
  census_<mode>_b<B>   library launches of one decoding on either route (torch's own kernels for the bookkeeping are not counted)
  read_images_per_s_b<B>   end-to-end `ASTER.read(images, "beam")` (rectification, encoder, decoder) on seeded images, same windows
  ids_equal_<mode>_b<B>    rows on which the two routes return the same ids up to the first EOS (near-ties may differ)
One process under the one outer `timeout -k 10`, as tools/bench_read.py: the routes alternate in it, so a time limit per GPU step would
have to be one per process.  Like that tool it borrows a helper from tests/ (tests/aster_ref.py: seeded weights and features)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", default="1,48")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tatt_amd
    from tatt_amd import aster, ops
    from tatt_amd.build import build
    import aster_ref as R
    build(verbose=False)
    dev = torch.device("cuda:0")
    info = aster.AsterInfo("all")
    eos = info.char2id[info.EOS]
    torch.manual_seed(7)
    model = R.scale_fc(R.perturb(tatt_amd.ASTER(rec_num_classes=info.rec_num_classes, eos=eos), 11)).to(dev).eval()
    head = model.decoder
    operands = aster.decoder_operands(head)
    res = {"bench": "aster", "repeats": a.repeats, "calls": a.calls, "device": torch.cuda.get_device_name(0), "steps": head.max_len_labels,
           "classes": head.num_classes}

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
        before = aster.LAUNCHES["one_launch"]
        try:
            fn()
        finally:
            ops.call = real
        return n[0] + aster.LAUNCHES["one_launch"] - before         # (tatt_attn_decode is called past ops.call: it may return 1)

    with torch.no_grad():
        for B in [int(v) for v in a.batches.split(",")]:
            x = R.features(B, seed=3).to(dev)
            for mode, m in (("beam", 2), ("greedy", 1)):
                fns = {"eager": lambda: aster.decode_eager(head, x, m, eos), "one_launch": lambda: aster.attn_decode(head, x, m, eos, operands=operands)}
                ids_e, ids_o = fns["eager"]()[0].cpu().numpy(), fns["one_launch"]()[0].cpu().numpy()
                tag = "%s_b%d" % (mode, B)
                res["ids_equal_" + tag] = "%d/%d" % (sum(p == q for p, q in zip(R.upto_eos(ids_e, eos), R.upto_eos(ids_o, eos))), B)
                res["census_" + tag] = {k: census(f) for k, f in fns.items()}
                times = alternate(fns)
                for k in fns:
                    res["%s_ms_%s" % (k, tag)] = span(times[k])
                res["disjoint_" + tag] = bool(max(times["one_launch"]) < min(times["eager"]))
            g = torch.Generator().manual_seed(5)
            img = (torch.rand(B, 3, 32, 128, generator=g) * 2 - 1).to(dev)
            times = alternate({"read": lambda: model.read(img, "beam")})
            res["read_ms_b%d" % B] = span(times["read"])
            res["read_images_per_s_b%d" % B] = round(B * 1e3 / statistics.median(times["read"]), 1)
            res["census_read_b%d" % B] = census(lambda: model.read(img, "beam"))
    tatt_amd.sync_check()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
