"""The word-segmentation kernel off the GPU: csrc/ctcwords.hip compiled for the CPU with the thread-per-lane stand-in of tools/words_host
(one host thread per lane, the cross-lane moves and the LDS maxima emulated behind barriers) as a STAND-ALONE program under
-fsanitize=address,undefined, run on the shapes of tests/test_words_device_gpu.py and held to the specification:
(a) its lp_out within the bar of the specification's log-soft-max, (b) `read.ctc_words_host` on its own lp_out equal to its record bit
for bit, the canary beyond the stated words intact, rows without a valid index untouched.  Nothing is loaded into this process.
It is a check for the BUILD machine (CPUs, no GPU); it is not run on a GPU machine, and it stops where LD_PRELOAD is set: a
sanitized program must be the first thing loaded, and the tool leaves that setting as it is.

    python tools/words_host_check.py [--keep DIR] [--lines-at-the-limit 1]

Exit status 0 and "host check clean" where every case holds and the sanitizers reported nothing."""
import argparse
import math
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FILL, EXTRA = -77, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run here, and keep the files")
    ap.add_argument("--lines-at-the-limit", type=int, default=1, help="lines of the lane-limit case (each is 16384 threads' worth of barriers)")
    a = ap.parse_args()
    if os.environ.get("LD_PRELOAD"):
        print("host check not run: LD_PRELOAD is set here.  The check is meant for the build machine, which has no GPU and preloads "
              "nothing; it leaves the setting as it is.")
        return 2
    from tatt_amd import read
    from tests.test_words import NEG, case_inputs, cases, degenerate_word_lines, log_softmax_rows, planted_lines
    work = a.keep or tempfile.mkdtemp(prefix="words_host_")
    os.makedirs(work, exist_ok=True)
    for name in ("ctcwords.hip", "ctc_lex.h", "ctc_f64.h"):
        shutil.copy(os.path.join(ROOT, "tatt_amd", "csrc", name), work)
    for name in ("common.h", "main.cpp"):
        shutil.copy(os.path.join(ROOT, "tools", "words_host", name), work)
    exe = os.path.join(work, "words_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-Wno-unknown-pragmas", "-pthread", os.path.join(work, "main.cpp"), "-o", exe], check=True)

    todo = []                                                        # (name, logits, lexicon, penalty, index, n_rows)
    for name in cases():
        x, lex, wp = case_inputs(name)
        if name == "lane-limit":
            x = x[:, :a.lines_at_the_limit]
        todo.append((name, x, lex, wp, list(range(x.shape[1])), x.shape[1]))
    x, _, lex = planted_lines(range(17))
    todo.append(("planted", x, lex, 0.0, list(range(17)), 17))
    x, lex, _ = degenerate_word_lines()
    todo.append(("degenerate", x, lex, 0.0, [8, -1, 6, 5, 9, 3], 9))
    for words in (["to", "day", "today", "a", "y"], ["today", "y", "to", "a", "day"]):
        todo.append(("ties", torch.zeros(9, 2, 27), read.Lexicon(words, alphabet="-abcdefghijklmnopqrstuvwxyz"), 0.0, [0, 1], 2))
    with open(os.path.join(work, "cases.bin"), "wb") as f:
        f.write(struct.pack("<i", len(todo)))
        for name, x, lex, wp, index, n_rows in todo:
            T, B, C = x.shape
            f.write(struct.pack("<12i", T, B, C, len(lex), *lex.counts, lex.n_codes, n_rows, read.words_record_words(T) + EXTRA, T, 1))
            f.write(struct.pack("<d", wp))
            f.write(lex.codes.astype("<i4").tobytes() + lex.table.astype("<i4").tobytes() + np.asarray(index, "<i4").tobytes())
            f.write(x.contiguous().numpy().astype("<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, os.path.join(work, "cases.bin"), os.path.join(work, "results.bin")], env=env, capture_output=True, text=True)
    sys.stderr.write(run.stderr)
    if run.returncode != 0 or "Sanitizer" in run.stderr or "runtime error" in run.stderr:
        print("host check FAILED: exit status %d" % run.returncode)
        return 1
    raw, off, bad = open(os.path.join(work, "results.bin"), "rb").read(), 0, 0
    for name, x, lex, wp, index, n_rows in todo:
        T, B, C = x.shape
        width = read.words_record_words(T)
        rc = struct.unpack_from("<i", raw, off)[0]
        off += 4
        rec = torch.from_numpy(np.frombuffer(raw, "<i4", n_rows * (width + EXTRA), off).reshape(n_rows, width + EXTRA).copy())
        off += 4 * n_rows * (width + EXTRA)
        lp = np.frombuffer(raw, "<f8", B * T * C, off).reshape(B, T, C)
        off += 8 * B * T * C
        assert rc == 0, (name, rc)
        dist = top = worst = 0.0
        for b in range(B):
            want = log_softmax_rows(x, b)
            if any(r is None for r in want) or not 0 <= index[b] < n_rows:
                continue
            wide = log_softmax_rows(x, b, np.longdouble)
            for r, w in zip(want, wide):
                for v, u in zip(r, w):
                    if v != NEG:
                        dist, top = max(dist, abs(float(np.longdouble(v) - u))), max(top, abs(v))
        bar = 4 * dist + 2.0 ** -52 * top
        for r in range(n_rows):
            if r not in index:
                assert bool((rec[r] == FILL).all()), (name, r)
        for b in range(B):
            r = index[b]
            if not 0 <= r < n_rows:
                assert bool((lp[b] == 12345.0).all()), (name, b)
                continue
            got = read.parse_words_records(rec[r:r + 1, :width].contiguous(), T)[0]
            want = log_softmax_rows(x, b)
            if any(row is None for row in want):
                assert got.flag == 1 and got.words == [] and math.isnan(got.logp) and bool(np.isnan(lp[b]).all()), (name, b)
                assert bool((rec[r, 4:] == FILL).all()), (name, b)
                continue
            for t in range(T):
                for c in range(C):
                    v, u = want[t][c], float(lp[b, t, c])
                    if v == NEG:
                        assert u == NEG, (name, b, t, c)
                    else:
                        assert abs(u - v) <= bar, (name, b, t, c, u, v, bar)
                        worst = max(worst, abs(u - v))
            spec = read.ctc_words_host(lp[b].tolist(), lex, wp)
            same = got.flag == 0 and struct.pack("<d", got.logp) == struct.pack("<d", spec.logp) and got.words == spec.words
            canary = bool((rec[r, 4 + 2 * len(spec.words):] == FILL).all())
            if not (same and canary):
                bad += 1
                print("MISMATCH %s line %d: %r against %r, canary %s" % (name, b, got, spec, canary))
        print("%-14s T %3d, n %2d, C %2d, K %4d, lanes %5d: bar %.3g, program - specification of lp %.3g, records bit-equal"
              % (name, T, B, C, len(lex), read.words_lanes(lex), bar, worst))
    assert off == len(raw)
    if not a.keep:
        shutil.rmtree(work)
    print("host check clean" if not bad else "host check FAILED: %d lines differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
