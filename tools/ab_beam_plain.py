"""The plain beam launch (tatt_ctc_beam_read) of this tree beside that of a baseline checkout in _base/ (a git worktree of an earlier
commit, built in place: see tools/ab_base.sh, which sets up the same _base/ but times bench.py, the training step, and so says nothing
about a decoding kernel).  Box-to-box variation is larger than most changes to one kernel, so the two trees alternate inside one call:
`--rounds` times, one fresh process per tree (each imports its OWN tatt_amd and loads its own library; this driver never opens the GPU).

    timeout -k 10 600 python tools/ab_beam_plain.py [--rounds 3] [--base _base]

Per process: seeded logits (randn * 3, C = 37) at (T, n) = (26, 48) and (256, 16), beam 8, nbest 4; one warm-up window, then 5 windows of
50 launches between device events; min / median / max in microseconds per launch, and a checksum over the first entry of every record
(the two trees must write the same words).  Prints one JSON line per process, then whether the ranges of the two trees overlap per shape:
overlap means "no change shown".  Reports only."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((26, 48), (256, 16))


def child(tree, name):
    sys.path.insert(0, tree)
    import torch
    from tatt_amd import read
    assert os.path.abspath(read.__file__).startswith(os.path.abspath(tree) + os.sep), read.__file__
    dev = torch.device("cuda:0")
    res = {"tree": name}
    for T, n in SHAPES:
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        rec = torch.empty(n, read.beam_record_words(T, 4), dtype=torch.int32, device=dev)
        ts = []
        for w in range(6):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                read.ctc_beam_read(x, index, rec, T, 8, 4)
            e1.record()
            e1.synchronize()
            if w:
                ts.append(e0.elapsed_time(e1) * 1e3 / 50)
        res["plain_us_T%d_n%d" % (T, n)] = {"min": round(min(ts), 2), "median": round(statistics.median(ts), 2), "max": round(max(ts), 2)}
        res["checksum_T%d" % T] = int(rec.cpu()[:, 2:8].to(torch.int64).sum())
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--base", default=os.path.join(ROOT, "_base"))
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    base = os.path.abspath(a.base)
    if not os.path.exists(os.path.join(base, "tatt_amd", "lib", "libtatt_hip.so")):
        sys.exit("no built baseline in %s: git worktree add _base <commit> && (cd _base && python -m tatt_amd.build)" % base)
    runs = {"base": [], "new": []}
    for _ in range(a.rounds):
        for name, tree in (("base", base), ("new", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, name], capture_output=True, text=True,
                                 timeout=180, cwd=tree)
            if out.returncode != 0:                                  # (nothing more is started on the GPU after a failure)
                sys.stderr.write(out.stderr)
                sys.exit("the %s tree's process ended with status %d" % (name, out.returncode))
            line = out.stdout.strip().splitlines()[-1]
            print(line)
            runs[name].append(json.loads(line))
    res = {"bench": "ab_beam_plain", "rounds": a.rounds}
    for T, n in SHAPES:
        k = "plain_us_T%d_n%d" % (T, n)
        lo = {s: min(r[k]["min"] for r in runs[s]) for s in runs}
        hi = {s: max(r[k]["max"] for r in runs[s]) for s in runs}
        res[k] = {s: [lo[s], hi[s]] for s in runs}
        res["ranges_overlap_T%d_n%d" % (T, n)] = bool(lo["new"] <= hi["base"] and lo["base"] <= hi["new"])
        res["same_words_T%d" % T] = len({r["checksum_T%d" % T] for s in runs for r in runs[s]}) == 1
    print(json.dumps(res))


if __name__ == "__main__":
    main()
