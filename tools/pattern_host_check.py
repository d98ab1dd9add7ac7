"""Pattern decoding off the GPU: csrc/ctcbeam.hip (the pattern instantiation) and csrc/ctcpat.hip compiled for the CPU with the
thread-per-lane stand-in of tools/words_host (one host thread per lane, the data-parallel-primitive moves, lane reads and ballots emulated
behind barriers) as a STAND-ALONE program under -fsanitize=address,undefined, run on the shapes of tests/test_pattern_device_gpu.py
through the entries tatt_ctc_beam_pattern_read and tatt_ctc_pattern_mass, on exactly sized heap buffers, and held to the specifications:
strings, lengths and order equal `read.ctc_beam_pattern_read_host`, logp and mass within the bars of the GPU test
(tests/test_pattern.py `pattern_bars`), `.*` equal to tatt_ctc_beam_read word for word, the canary beyond the stated words intact, rows
without a valid index untouched, refused geometries left alone, no LDS byte written beyond a launch's own.  Nothing is loaded into this
process.  It is a check for the BUILD machine (CPUs, no GPU), to be run before the first launch of a changed kernel; it is not run on a GPU
machine, and it stops where LD_PRELOAD is set: a sanitized program must be the first thing loaded, and the tool leaves that setting as it
is.

    python tools/pattern_host_check.py [--keep DIR] [--rows N]

--rows N runs at most N lines of every case (a line of 256 steps over 64 states is some 10^6 barriers of 64 threads).
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
    from tests.test_pattern import PATTERN_CASES, flagged_lines, pattern_bars, pattern_case
    work = a.keep or tempfile.mkdtemp(prefix="pattern_host_")
    csrc, tools = os.path.join(ROOT, "tatt_amd", "csrc"), os.path.join(ROOT, "tools")
    for sub, files in (("beam", ((csrc, "ctcbeam.hip", None), (csrc, "ctc_f64.h", None), (tools, "beam_lm_host/common.h", "common.h"),
                                 (tools, "words_host/common.h", "words_common.h"), (tools, "pattern_host/beam.cpp", None))),
                       ("mass", ((csrc, "ctcpat.hip", None), (csrc, "ctc_f64.h", None), (tools, "words_host/common.h", "common.h"),
                                 (tools, "pattern_host/main.cpp", None)))):
        os.makedirs(os.path.join(work, sub), exist_ok=True)
        for base, name, as_ in files:
            shutil.copy(os.path.join(base, name), os.path.join(work, sub, as_ or os.path.basename(name)))
    exe = os.path.join(work, "pattern_host")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
             "-Wno-unknown-pragmas", "-pthread"]
    objs = []
    for sub, src in (("beam", "beam.cpp"), ("mass", "main.cpp")):
        objs.append(os.path.join(work, sub, src[:-4] + ".o"))
        subprocess.run(["g++"] + flags + ["-x", "c++", "-c", os.path.join(work, sub, src), "-o", objs[-1]], check=True)
    subprocess.run(["g++"] + flags + objs + ["-o", exe], check=True)

    # (name, logits, pattern, beam, nbest, index, n_rows, cap, refused, plain)
    todo = []
    for case in PATTERN_CASES:
        T, B, C, beam, nbest, s, seed, spec, alphabet = case
        x, pat, _, _ = pattern_case(case)
        if a.rows:
            x = x[:, :a.rows]
        n = x.shape[1]
        todo.append(("T%d-C%d-beam%d-S%d" % (T, C, beam, pat.n_states), x, pat, beam, nbest, list(range(n)), n, T, False, False))
    x, spec = flagged_lines()
    todo.append(("flagged", x, read.Pattern(spec, "-abc"), 8, 8, list(range(6)), 6, 6, False, False))
    x, pat, _, _ = pattern_case(PATTERN_CASES[2])
    todo.append(("dot-star", x, read.Pattern(".*"), 8, 4, [0, 1, 2], 3, 26, False, True))
    todo.append(("scattered", x, pat, 8, 4, [4, -1, 1], 6, 29, False, False))                  # an odd cap, rows out of order, one dropped
    todo.append(("no-row", x, pat, 8, 4, [-1, 6, 2 ** 30], 6, 29, False, False))
    for why in ("states", "no-states", "row", "nbest"):
        todo.append(("refused-" + why, x, pat, 4 if why == "nbest" else 8, 8 if why == "nbest" else 4, [0, 1, 2], 3, 26, why, False))

    def geometry(item):
        name, x, pat, beam, nbest, index, n_rows, cap, refused, plain = item
        words = read.beam_record_words(cap, nbest)
        st_rec, st_mass = words + EXTRA, read.PATTERN_MASS_WORDS + EXTRA
        if refused == "row":
            st_rec, st_mass = words - 1, read.PATTERN_MASS_WORDS - 1
        return words, st_rec, st_mass
    with open(os.path.join(work, "cases.bin"), "wb") as f:
        f.write(struct.pack("<i", len(todo)))
        for item in todo:
            name, x, pat, beam, nbest, index, n_rows, cap, refused, plain = item
            T, B, C = x.shape
            words, st_rec, st_mass = geometry(item)
            S = 65 if refused == "states" else 0 if refused == "no-states" else pat.n_states
            table = np.full((max(S, pat.n_states), C), 255, np.uint8)
            table[:pat.n_states] = pat.table_for(C)
            accept = np.zeros(max(S, pat.n_states), np.uint8)
            accept[:pat.n_states] = pat.accept
            f.write(struct.pack("<12i", T, B, C, beam, nbest, S, n_rows, st_rec, cap, st_mass, int(plain), 0))
            f.write(table[:S].tobytes() + accept[:S].tobytes() + np.asarray(index, "<i4").tobytes())
            f.write(x.contiguous().numpy().astype("<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, os.path.join(work, "cases.bin"), os.path.join(work, "results.bin")], env=env, capture_output=True, text=True)
    sys.stderr.write(run.stderr)
    if run.returncode != 0 or "Sanitizer" in run.stderr or "runtime error" in run.stderr:
        print("host check FAILED: exit status %d" % run.returncode)
        return 1
    raw, off, bad = open(os.path.join(work, "results.bin"), "rb").read(), 0, 0

    def block(n_rows, stride):
        nonlocal off
        rc = struct.unpack_from("<i", raw, off)[0]
        buf = torch.from_numpy(np.frombuffer(raw, "<i4", n_rows * stride, off + 4).reshape(n_rows, stride).copy())
        off += 4 + 4 * n_rows * stride
        return rc, buf
    for item in todo:
        name, x, pat, beam, nbest, index, n_rows, cap, refused, plain = item
        T, B, C = x.shape
        words, st_rec, st_mass = geometry(item)
        rc, rec = block(n_rows, st_rec)
        rm, mass = block(n_rows, st_mass)
        if refused:
            ok = rc == 1 and bool((rec == FILL).all()) and (refused == "nbest" or (rm == 1 and bool((mass == FILL).all())))
            print("%-24s refused (%s): return codes %d, %d, the outputs %s" % (name, refused, rc, rm, "untouched" if ok else "WRITTEN"))
            bad += not ok
            continue
        assert rc == 0 and rm == 0, (name, rc, rm)
        if plain:
            rp, other = block(n_rows, st_rec)
            same = rp == 0 and bool((other == rec).all())
            print("%-24s the record of tatt_ctc_beam_read, word for word: %s" % (name, "equal" if same else "DIFFERENT"))
            bad += not same
        want = read.ctc_beam_pattern_read_host(x, pat, beam, nbest, details=True)
        wide = read.ctc_beam_pattern_read_host(x, pat, beam, nbest, real=np.longdouble)
        bar, mbar, _, _ = pattern_bars(T, pat.n_states, C, want, wide)
        worst = worst_m = 0.0
        for r in range(n_rows):
            if r not in index:
                assert bool((rec[r] == FILL).all()) and bool((mass[r] == FILL).all()), (name, r)
        es = read.beam_entry_words(cap)
        for b in range(B):
            r = index[b]
            if not 0 <= r < n_rows:
                continue
            got = read.parse_beam_records(rec[r:r + 1, :words].contiguous(), cap, nbest)[0]
            gm = read.parse_pattern_mass(mass[r:r + 1])[0]
            w = want[b]
            same = got.flag == w.flag == gm.flag and [e[0] for e in got.entries] == [e[0] for e in w.entries]
            err = max([abs(g[1] - e[1]) for g, e in zip(got.entries, w.entries)], default=0.0)
            if w.flag:
                em = 0.0 if np.isnan(gm.mass) else float("inf")
            else:
                em = 0.0 if gm.mass == w.mass else abs(gm.mass - w.mass)
            canary = bool((rec[r, 2 + len(w.entries) * es:] == FILL).all()) and bool((mass[r, read.PATTERN_MASS_WORDS:] == FILL).all())
            worst, worst_m = max(worst, err), max(worst_m, em)
            if not (same and canary and err <= bar and em <= mbar):
                bad += 1
                print("MISMATCH %s line %d: %r %r against %r, canary %s, |logp - specification| %.3g, bar %.3g, mass %.3g, bar %.3g"
                      % (name, b, got, gm, w, canary, err, bar, em, mbar))
        print("%-24s T %3d, n %2d, C %2d, beam %2d, S %2d: logp bar %.3g, program - specification %.3g; mass bar %.3g, program - "
              "specification %.3g; smallest margin %.3g; strings equal" % (name, T, B, C, beam, pat.n_states, bar, worst, mbar, worst_m,
                                                                          min((w.margin for w in want if not w.flag), default=float("inf"))))
    assert off == len(raw)
    if not a.keep:
        shutil.rmtree(work)
    print("host check clean" if not bad else "host check FAILED: %d lines differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
