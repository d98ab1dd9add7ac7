"""Forced alignment beside the greedy and the beam decoding (csrc/ctcalign.hip, csrc/read.hip, csrc/ctcbeam.hip): the launches alone on
given logits, and `tatt_amd.read.LineReader.read` with and without locate=True, in one process, alternating.  Reports only (one JSON
line); asserts nothing but that every line was aligned.

    python tools/bench_align.py [--out FILE]

The measuring runs in ONE child process under `timeout -k 10` (the parent never opens the GPU); 5 repeats, min / median / max.
Launches alone, on seeded logits (randn * 3, C = 37) with packed strings of about T / 3 characters (T // 3 - 1 .. T // 3 + 1, no equal
neighbours), at (T, n) = (26, 48) and (256, 16): `align`: tatt_ctc_align, `align_lp`: the same launch writing lp_out, `align_no_walk`:
the same strings ending in a class whose logits are all -inf, so that the recursion runs as before and finds no alignment: no walk
back, no sums -- the difference to `align` is what the walk and the sums cost; `greedy`, `beam8` (nbest 4), and `forward`: the chunk's
CRNN forward -- device time from events around 20 calls, microseconds per call; per repeat every candidate runs one such window, in an
order that rotates with the repeat.  `align_vs_<other>_*`: "below" / "above" where the two ranges are disjoint, "overlap" otherwise.
The reader: the 16 lines of tools/bench_read.py's `lines16` case, `LineReader.read(...).result()` under decode="greedy" and "beam"
(beam 8, nbest 4), each with and without locate=True (with it `locations()` is taken too), host time of a window of 5 calls that ends
in a device synchronise, milliseconds per call, same alternation.  TSRN and CRNN with seeded weights; batch_size 48."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, CALLS, WARMUP, LIMIT = 5, 20, 1, 540


def child(out):
    import numpy as np
    import torch
    from PIL import Image
    import tatt_amd
    from tatt_amd import read
    from tatt_amd.build import build
    from tatt_amd.infer import SuperResolver
    from oracle.fixtures import randomize_state_dict
    from tests.pil_resample_ref import make_image
    build(verbose=False)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    gen.load_state_dict(randomize_state_dict(gen.state_dict()))
    gen = gen.to(dev).eval()
    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    crnn.load_state_dict(randomize_state_dict(crnn.state_dict(), seed=11))
    crnn = crnn.to(dev).eval()
    res = {"bench": "align", "repeats": REPEATS, "calls": CALLS, "device": torch.cuda.get_device_name(0), "limits": read.align_limits()}
    span = lambda ts, nd=2: {"min": round(min(ts), nd), "median": round(statistics.median(ts), nd), "max": round(max(ts), nd)}

    def alternate(fns, window):
        names = list(fns)
        for k in names:
            for _ in range(WARMUP):
                window(fns[k])
        times = {k: [] for k in names}
        for r in range(REPEATS):
            rot = r % len(names)
            for k in names[rot:] + names[:rot]:
                times[k].append(window(fns[k]))
        return times

    def device_window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / CALLS

    def versus(x, y):
        return "below" if max(x) < min(y) else "above" if min(x) > max(y) else "overlap"

    # ---- the launches alone ----
    reader = read.LineReader(crnn, batch_size=48)
    for T, n in ((26, 48), (256, 16)):
        rng = random.Random(T)
        strings = []
        for _ in range(n):
            s = []
            for _ in range(T // 3 + rng.randint(-1, 1)):
                c = rng.randrange(1, 36)
                while s and c == s[-1]:
                    c = rng.randrange(1, 36)
                s.append(c)
            strings.append(s)
        cap_len = max(len(s) for s in strings)
        x = (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
        dead = x.clone()
        dead[:, :, 36] = float("-inf")
        img = torch.rand(n, 1, 32, 4 * (T - 1), generator=torch.Generator().manual_seed(n)).to(dev)
        assert reader.forward(img).shape == (T, n, 37)
        index = torch.arange(n, dtype=torch.int32).to(dev)
        table = torch.from_numpy(read.pack_strings(strings, cap_len)).to(dev)
        table_dead = torch.from_numpy(read.pack_strings([s[:-1] + [36] for s in strings], cap_len)).to(dev)
        greedy_rec = torch.empty(n, 3 * T + 2, dtype=torch.int32, device=dev)
        beam_rec = torch.empty(n, read.beam_record_words(T, 4), dtype=torch.int32, device=dev)
        rec = torch.empty(n, read.align_record_words(cap_len), dtype=torch.int32, device=dev)
        rec_dead = torch.empty(n, read.align_record_words(cap_len), dtype=torch.int32, device=dev)
        lp = torch.empty(n, T, 37, dtype=torch.float64, device=dev)
        fns = {"align": lambda: read.ctc_align(x, index, table, 0, 2, -1, rec, 0, cap_len),
               "align_lp": lambda: read.ctc_align(x, index, table, 0, 2, -1, rec, 0, cap_len, lp),
               "align_no_walk": lambda: read.ctc_align(dead, index, table_dead, 0, 2, -1, rec_dead, 0, cap_len),
               "greedy": lambda: read.ctc_greedy_read(x, index, greedy_rec, T),
               "beam8": lambda: read.ctc_beam_read(x, index, beam_rec, T, 8, 4),
               "forward": lambda: reader.forward(img)}
        times = alternate(fns, device_window)
        tag = "T%d_n%d" % (T, n)
        for k in fns:
            res["%s_us_%s" % (k, tag)] = span(times[k])
        res["align_us_per_step_%s" % tag] = span([t / T for t in times["align"]], 3)
        for k in ("align_no_walk", "greedy", "beam8", "forward"):
            res["align_vs_%s_%s" % (k, tag)] = versus(times["align"], times[k])
        got = read.parse_align_records(rec.cpu(), cap_len)
        assert all(g.flag == 0 and len(g.spans) == len(s) for g, s in zip(got, strings))
        assert all(g.flag == 0 and g.spans == [] and g.logp == float("-inf") for g in read.parse_align_records(rec_dead.cpu(), cap_len))
        res["characters_per_line_%s" % tag] = round(sum(len(s) for s in strings) / n, 1)

    # ---- the reader with and without locate ----
    rng = np.random.default_rng(7)
    keep = SuperResolver(gen, batch_size=48, long_lines=True, keep_sr=True)
    imgs = [Image.fromarray(make_image(rng, 40, w, i % 3), "RGB") for i, w in enumerate((128, 300, 600, 1200) * 4)]
    p = keep(imgs)
    pending = keep.exporter.lines(p.sr, p.lines, 2)
    buf, rows = pending.line_canvases
    buf = buf.clone()
    readers = {"greedy": reader, "greedy_locate": read.LineReader(crnn, batch_size=48, locate=True),
               "beam": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4),
               "beam_locate": read.LineReader(crnn, batch_size=48, decode="beam", beam=8, nbest=4, locate=True)}
    calls = max(1, CALLS // 4)

    def host_window(fn):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    def run(r):
        q = r.read(buf, rows, 2)
        return (q.result(), q.locations()) if r.locate else (q.result(), None)
    fns = {k: (lambda r=r: run(r)) for k, r in readers.items()}
    first = {k: fn() for k, fn in fns.items()}
    assert all(len(v[0]) == 16 for v in first.values()) and all(len(first[k][1]) == 16 for k in ("greedy_locate", "beam_locate"))
    assert all(l.flag in (0, 2) for k in ("greedy_locate", "beam_locate") for l in first[k][1])
    res["lines"] = len(rows)
    times = alternate(fns, host_window)
    for k in fns:
        res["reader_%s_ms" % k] = span(times[k], 3)
    for k in ("greedy", "beam"):
        res["reader_%s_locate_vs_plain" % k] = versus(times[k + "_locate"], times[k])
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.out)
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + (["--out", a.out] if a.out else [])
    rc = subprocess.run(cmd, cwd=ROOT).returncode
    if rc != 0:
        print("bench_align: the measuring step ended with status %d; nothing more is started" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
