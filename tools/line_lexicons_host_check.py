"""The per-line lexicon kernels off the GPU: csrc/ctclexp.hip compiled for the CPU with the thread-per-lane stand-in of tools/words_host
(one host thread per lane, the cross-lane moves emulated behind barriers; tools/line_lexicons_host/main.cpp is the program) as a
STAND-ALONE program under -fsanitize=address,undefined, run through its two entries on exactly sized heap buffers on the cases of
tests/test_line_lexicons_device_gpu.py (tests/test_line_lexicons.py CASES, the corrupt tables beside clean tiles, scattered record rows)
and held to the specification: every finite score within the case's bar, -inf and NaN equal as such, entries, order and flags equal,
logz within bar + K x 2^-52, the fill beyond every line's count and in rows without a valid index intact, and the corrupt tables
writing exactly what the clean ones write.  Nothing is loaded into this process.
It is a check for the BUILD machine (CPUs, no GPU); it is not run on a GPU machine, and it stops where LD_PRELOAD is set: a
sanitized program must be the first thing loaded, and the tool leaves that setting as it is.

    python tools/line_lexicons_host_check.py [--keep DIR]

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

FILL, SCORE_FILL, EXTRA = -77, 12345.0, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run here, and keep the files")
    a = ap.parse_args()
    if os.environ.get("LD_PRELOAD"):
        print("host check not run: LD_PRELOAD is set here.  The check is meant for the build machine, which has no GPU and preloads "
              "nothing; it leaves the setting as it is.")
        return 2
    from tatt_amd import read
    from tests.test_line_lexicons import CASES, compare_with_spec, corrupt_tables, line_case
    work = a.keep or tempfile.mkdtemp(prefix="line_lexicons_host_")
    os.makedirs(work, exist_ok=True)
    for name in ("ctclexp.hip", "ctc_lex.h", "ctc_f64.h"):
        shutil.copy(os.path.join(ROOT, "tatt_amd", "csrc", name), work)
    shutil.copy(os.path.join(ROOT, "tools", "words_host", "common.h"), work)
    shutil.copy(os.path.join(ROOT, "tools", "line_lexicons_host", "main.cpp"), work)
    exe = os.path.join(work, "line_lexicons_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-Wno-unknown-pragmas", "-pthread", os.path.join(work, "main.cpp"), "-o", exe], check=True)

    todo = []                                                        # (what, case, tables, index, n_rows)
    for name in CASES:
        x, lex, want, dec, bar, dist = line_case(name)
        n = x.shape[1]
        todo.append((name, name, lex.pack(range(n)), list(range(n)), n))
    x, lex = line_case("reader-T")[:2]
    todo.append(("corrupt tables", "reader-T", corrupt_tables(lex, 5), list(range(5)), 5))
    todo.append(("scattered rows", "reader-T", lex.pack(range(5)), [6, -1, 0, 7, 3], 7))
    with open(os.path.join(work, "cases.bin"), "wb") as f:
        f.write(struct.pack("<i", len(todo)))
        for what, name, (tiles, pairs, counts), index, n_rows in todo:
            x, lex = line_case(name)[:2]
            T, B, C = x.shape
            nbest, most = CASES[name][5], max(1, int(counts.max()))
            f.write(struct.pack("<12i", T, B, C, lex.table.shape[0], lex.n_codes, len(tiles), len(pairs), most, most + EXTRA, nbest, n_rows,
                                read.lexicon_record_words(nbest) + EXTRA))
            for arr in (lex.codes, lex.table, tiles, pairs, counts, np.asarray(index)):
                f.write(np.ascontiguousarray(arr).astype("<i4").tobytes())
            f.write(x.contiguous().numpy().astype("<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, os.path.join(work, "cases.bin"), os.path.join(work, "results.bin")], env=env, capture_output=True, text=True)
    sys.stderr.write(run.stderr)
    if run.returncode != 0 or "Sanitizer" in run.stderr or "runtime error" in run.stderr:
        print("host check FAILED: exit status %d" % run.returncode)
        return 1
    raw, off, clean = open(os.path.join(work, "results.bin"), "rb").read(), 0, {}
    for what, name, (tiles, pairs, counts), index, n_rows in todo:
        x, lex, want, dec, bar, dist = line_case(name)
        T, B, C = x.shape
        nbest, most = CASES[name][5], max(1, int(counts.max()))
        width = read.lexicon_record_words(nbest)
        rc, rc2 = struct.unpack_from("<ii", raw, off)
        off += 8
        scores = torch.from_numpy(np.frombuffer(raw, "<f8", B * (most + EXTRA), off).reshape(B, most + EXTRA).copy())
        off += 8 * B * (most + EXTRA)
        rec = torch.from_numpy(np.frombuffer(raw, "<i4", n_rows * (width + EXTRA), off).reshape(n_rows, width + EXTRA).copy())
        off += 4 * n_rows * (width + EXTRA)
        assert (rc, rc2) == (0, 0), (what, rc, rc2)
        assert bool((rec[:, width:] == FILL).all()), what
        for r in range(n_rows):
            if r not in index:
                assert bool((rec[r] == FILL).all()), (what, r)       # rows without a valid index keep their fill
        rows = [r for r in index if 0 <= r < n_rows]
        lines = [b for b, r in enumerate(index) if 0 <= r < n_rows]
        got = read.parse_lexicon_records(rec[rows][:, :width].contiguous(), nbest)
        for g, r in zip(got, rows):                                  # words of entries that do not exist are not written
            assert bool((rec[r, 4 + 4 * len(g.entries):] == FILL).all()), (what, r)
        if what == name:
            worst = compare_with_spec(name, scores, got)
            clean[name] = (scores, rec)
            print("%-10s T %3d, n %d, C %2d, words %s, union %d, %d tiles: bar %.3g (float64 - longdouble %.3g), program - specification "
                  "%.3g, smallest margin %.3g" % (name, T, B, C, counts.tolist(), len(lex.union), len(tiles), bar, dist, worst,
                                                  min(d.margin for d in dec)))
        elif what == "corrupt tables":                               # exactly what the clean tables wrote, fill included
            assert torch.equal(scores.view(torch.int64), clean[name][0].view(torch.int64)) and torch.equal(rec, clean[name][1]), what
            print("%-10s %d tiles and %d pairs, the corrupt ones among them: scores and records bit-equal to the clean tables', fill intact"
                  % (what, len(tiles), len(pairs)))
        else:
            assert torch.equal(scores.view(torch.int64), clean[name][0].view(torch.int64)), what
            for b, r in zip(lines, rows):
                assert torch.equal(rec[r], clean[name][1][b]), (what, b, r)
            print("%-10s index %s into %d rows: the valid rows equal the clean ones, the others keep their fill" % (what, index, n_rows))
    assert off == len(raw)
    if not a.keep:
        shutil.rmtree(work)
    print("host check clean")
    return 0


if __name__ == "__main__":
    sys.exit(main())
