"""The beam kernel off the GPU, with and without the language model: csrc/ctcbeam.hip compiled for the CPU with the thread-per-lane
stand-in of tools/words_host (one host thread per lane, the data-parallel-primitive moves, lane reads and ballots emulated behind
barriers; tools/beam_lm_host adds what this kernel needs on top) as a STAND-ALONE program under -fsanitize=address,undefined, run on the
shapes of tests/test_beam_lm_device_gpu.py through both entries, on exactly sized heap buffers, and held to the specifications:
strings, lengths and order equal `read.ctc_beam_lm_read_host` / `read.ctc_beam_read_host`, the 64 bits of every lm equal the
specification's, logp within the bar of the GPU tests (4 x |float64 - longdouble| of the specification + T x 2^-52 x max |logp|), the
canary beyond the stated words intact, rows without a valid index untouched, refused geometries left alone.  Nothing is loaded into this
process.  It is a check for the BUILD machine (CPUs, no GPU); it is not run on a GPU machine, and it stops where LD_PRELOAD is set: a
sanitized program must be the first thing loaded, and the tool leaves that setting as it is.

    python tools/beam_lm_host_check.py [--keep DIR] [--rows N]

--rows N runs at most N lines of every case (a line of 256 steps is some 10^5 barriers of 64 threads).
Exit status 0 and "host check clean" where every case holds and the sanitizers reported nothing."""
import argparse
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
    ap.add_argument("--rows", type=int, default=0, help="at most this many lines of every case (0: all)")
    a = ap.parse_args()
    if os.environ.get("LD_PRELOAD"):
        print("host check not run: LD_PRELOAD is set here.  The check is meant for the build machine, which has no GPU and preloads "
              "nothing; it leaves the setting as it is.")
        return 2
    from tatt_amd import read
    from tests.test_beam_lm import LM_CASES, flagged_lines, lm_case, lm_table, tie_tables
    work = a.keep or tempfile.mkdtemp(prefix="beam_lm_host_")
    os.makedirs(work, exist_ok=True)
    for name in ("ctcbeam.hip", "ctc_f64.h"):
        shutil.copy(os.path.join(ROOT, "tatt_amd", "csrc", name), work)
    shutil.copy(os.path.join(ROOT, "tools", "words_host", "common.h"), os.path.join(work, "words_common.h"))
    for name in ("common.h", "main.cpp"):
        shutil.copy(os.path.join(ROOT, "tools", "beam_lm_host", name), work)
    exe = os.path.join(work, "beam_lm_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-Wno-unknown-pragmas", "-pthread", os.path.join(work, "main.cpp"), "-o", exe], check=True)

    # (name, logits, lm or None, weight, bonus, beam, nbest, index, n_rows, cap, refused)
    todo = []
    for case in LM_CASES:
        T, B, C, beam, nbest, order, s, weight, bonus, seed = case
        x, lm, _ = lm_case(case)
        if a.rows:
            x = x[:, :a.rows]
        n = x.shape[1]
        todo.append(("T%d-C%d-beam%d-order%d" % (T, C, beam, order), x, lm, weight, bonus, beam, nbest, list(range(n)), n, T, False))
        todo.append(("T%d-C%d-beam%d-plain" % (T, C, beam), x, None, 0.0, 0.0, beam, nbest, list(range(n)), n, T, False))
    for lm, _, _ in tie_tables():
        todo.append(("ties-order%d" % lm.order, torch.zeros(2, 2, 4), lm, 1.0, 0.0, 5, 5, [0, 1], 2, 2, False))
    x, _ = flagged_lines()
    todo.append(("flagged", x, lm_table(4, 2, 40), .5, 0.0, 8, 8, list(range(6)), 6, 6, False))
    todo.append(("flagged-plain", x, None, 0.0, 0.0, 8, 8, list(range(6)), 6, 6, False))
    x, lm, _ = lm_case(LM_CASES[2])
    todo.append(("scattered", x, lm, .5, 0.0, 8, 4, [4, -1, 1], 6, 29, False))               # an odd cap, rows out of order, one dropped
    todo.append(("no-row", x, lm, .5, 0.0, 8, 4, [-1, 6, 2 ** 30], 6, 29, False))
    todo.append(("refused-order", x, lm, .5, 0.0, 8, 4, [0, 1, 2], 3, 26, "order"))
    todo.append(("refused-classes", x, lm, .5, 0.0, 8, 4, [0, 1, 2], 3, 26, "classes"))
    todo.append(("refused-row", x, lm, .5, 0.0, 8, 4, [0, 1, 2], 3, 26, "row"))
    todo.append(("refused-nbest", x, lm, .5, 0.0, 4, 8, [0, 1, 2], 3, 26, "nbest"))

    def width(lm, cap, nbest):
        return read.beam_lm_record_words(cap, nbest) if lm is not None else read.beam_record_words(cap, nbest)
    with open(os.path.join(work, "cases.bin"), "wb") as f:
        f.write(struct.pack("<i", len(todo)))
        for name, x, lm, weight, bonus, beam, nbest, index, n_rows, cap, refused in todo:
            T, B, C = x.shape
            table = lm.increments(weight, bonus).reshape(-1) if lm is not None else np.zeros(0)
            order, st_rec = lm.order if lm is not None else 0, width(lm, cap, max(nbest, 1)) + EXTRA
            if refused == "row":
                st_rec = width(lm, cap, nbest) - 1
            f.write(struct.pack("<12i", T, B, C, beam, nbest, 4 if refused == "order" else order, int(lm is not None), n_rows, st_rec, cap,
                                table.size, C + 1 if refused == "classes" else C))
            f.write(table.astype("<f8").tobytes() + np.asarray(index, "<i4").tobytes())
            f.write(x.contiguous().numpy().astype("<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, os.path.join(work, "cases.bin"), os.path.join(work, "results.bin")], env=env, capture_output=True, text=True)
    sys.stderr.write(run.stderr)
    if run.returncode != 0 or "Sanitizer" in run.stderr or "runtime error" in run.stderr:
        print("host check FAILED: exit status %d" % run.returncode)
        return 1
    raw, off, bad = open(os.path.join(work, "results.bin"), "rb").read(), 0, 0
    for name, x, lm, weight, bonus, beam, nbest, index, n_rows, cap, refused in todo:
        T, B, C = x.shape
        st_rec = width(lm, cap, nbest) - 1 if refused == "row" else width(lm, cap, max(nbest, 1)) + EXTRA
        rc = struct.unpack_from("<i", raw, off)[0]
        off += 4
        rec = torch.from_numpy(np.frombuffer(raw, "<i4", n_rows * st_rec, off).reshape(n_rows, st_rec).copy())
        off += 4 * n_rows * st_rec
        if refused:
            ok = rc == 1 and bool((rec == FILL).all())
            print("%-24s refused (%s): return code %d, the record %s" % (name, refused, rc, "untouched" if ok else "WRITTEN"))
            bad += not ok
            continue
        assert rc == 0, (name, rc)
        if lm is not None:
            want = read.ctc_beam_lm_read_host(x, lm, beam, nbest, weight, bonus, details=True)
            wide = read.ctc_beam_lm_read_host(x, lm, beam, nbest, weight, bonus, real=np.longdouble)
        else:
            want = read.ctc_beam_read_host(x, beam, nbest, details=True)
            wide = read.ctc_beam_read_host(x, beam, nbest, real=np.longdouble)
        dist = top = worst = 0.0
        for w, l in zip(want, wide):
            for e, g in zip(w.entries, l.entries):
                dist, top = max(dist, abs(float(np.longdouble(e[1]) - g[1]))), max(top, abs(e[1]))
        bar = 4 * dist + T * 2.0 ** -52 * top
        words = width(lm, cap, nbest)
        for r in range(n_rows):
            if r not in index:
                assert bool((rec[r] == FILL).all()), (name, r)
        for b in range(B):
            r = index[b]
            if not 0 <= r < n_rows:
                continue
            row = rec[r:r + 1, :words].contiguous()
            got = (read.parse_beam_lm_records if lm is not None else read.parse_beam_records)(row, cap, nbest)[0]
            w = want[b]
            es = read.beam_lm_entry_words(cap) if lm is not None else read.beam_entry_words(cap)
            same = got.flag == w.flag and [e[0] for e in got.entries] == [e[0] for e in w.entries]
            if lm is not None:
                same = same and [struct.pack("<d", e[2]) for e in got.entries] == [struct.pack("<d", e[2]) for e in w.entries]
            err = max([abs(g[1] - e[1]) for g, e in zip(got.entries, w.entries)], default=0.0)
            canary = bool((rec[r, 2 + len(w.entries) * es:] == FILL).all())
            worst = max(worst, err)
            if not (same and canary and err <= bar):
                bad += 1
                print("MISMATCH %s line %d: %r against %r, canary %s, |logp - specification| %.3g, bar %.3g" % (name, b, got, w, canary, err, bar))
        print("%-24s T %3d, n %2d, C %2d, beam %2d: bar %.3g, program - specification of logp %.3g, smallest margin %.3g, strings%s equal"
              % (name, T, B, C, beam, bar, worst, min((w.margin for w in want if not w.flag), default=float("inf")),
                 " and the bits of lm" if lm is not None else ""))
    assert off == len(raw)
    if not a.keep:
        shutil.rmtree(work)
    print("host check clean" if not bad else "host check FAILED: %d lines differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
