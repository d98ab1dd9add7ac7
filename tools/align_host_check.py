"""The forced-alignment kernel off the GPU: csrc/ctcalign.hip compiled for the CPU with the thread-per-lane stand-in of tools/words_host
(one host thread per lane, the cross-lane moves emulated behind barriers) and tools/align_host/main.cpp as a STAND-ALONE program under
-fsanitize=address,undefined, run on the launches of tests/test_align_device_gpu.py (tests/test_align.py `launches`) and held to the
specification: (a) its lp_out within the bar of the specification's log-soft-max, (b) every record row equal to the row before the
launch with the alignment part replaced by `read.ctc_align_host` on its own lp_out, bit for bit -- the canary beyond the stated
characters, the decode part and the rows without a valid index untouched.  Nothing is loaded into this process.
It is a check for the BUILD machine (CPUs, no GPU); it is not run on a GPU machine, and it stops where LD_PRELOAD is set: a
sanitized program must be the first thing loaded, and the tool leaves that setting as it is.

    python tools/align_host_check.py [--keep DIR] [--lines-at-the-limit 2]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run here, and keep the files")
    ap.add_argument("--lines-at-the-limit", type=int, default=2, help="lines of the case at T = 256, L = 127")
    a = ap.parse_args()
    if os.environ.get("LD_PRELOAD"):
        print("host check not run: LD_PRELOAD is set here.  The check is meant for the build machine, which has no GPU and preloads "
              "nothing; it leaves the setting as it is.")
        return 2
    from tests.test_align import launches, stage_a, stage_b
    work = a.keep or tempfile.mkdtemp(prefix="align_host_")
    os.makedirs(work, exist_ok=True)
    for name in ("ctcalign.hip", "ctc_lex.h", "ctc_f64.h"):
        shutil.copy(os.path.join(ROOT, "tatt_amd", "csrc", name), work)
    shutil.copy(os.path.join(ROOT, "tools", "words_host", "common.h"), work)
    shutil.copy(os.path.join(ROOT, "tools", "align_host", "main.cpp"), work)
    exe = os.path.join(work, "align_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-Wno-unknown-pragmas", "-pthread", os.path.join(work, "main.cpp"), "-o", exe], check=True)

    todo = launches(a.lines_at_the_limit)
    with open(os.path.join(work, "cases.bin"), "wb") as f:
        f.write(struct.pack("<i", len(todo)))
        for l in todo:
            x, before, table = l["x"], l["before"], l["table"]
            T, B, C = x.shape
            assert x.storage_offset() == 0
            store = x.contiguous().reshape(-1) if x.is_contiguous() else torch.as_strided(x, (x.untyped_storage().nbytes() // 4,), (1,), 0)
            src = before if table is None else table
            f.write(struct.pack("<18i", T, B, C, before.shape[0], before.shape[1], l["rec_at"], l["cap_len"], src.shape[0], src.shape[1],
                                l["len_at"], l["cls_at"], l["gate_at"], int(table is None), 1, *x.stride(), store.numel()))
            f.write(np.asarray(l["index"], "<i4").tobytes() + before.numpy().astype("<i4").tobytes())
            if table is not None:
                f.write(table.numpy().astype("<i4").tobytes())
            f.write(store.numpy().astype("<f4").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, os.path.join(work, "cases.bin"), os.path.join(work, "results.bin")], env=env, capture_output=True, text=True)
    sys.stderr.write(run.stderr)
    if run.returncode != 0 or "Sanitizer" in run.stderr or "runtime error" in run.stderr:
        print("host check FAILED: exit status %d" % run.returncode)
        return 1
    raw, off, bad = open(os.path.join(work, "results.bin"), "rb").read(), 0, 0
    for l in todo:
        x, before = l["x"], l["before"]
        T, B, C = x.shape
        n_rows, width = before.shape
        rc = struct.unpack_from("<i", raw, off)[0]
        off += 4
        after = torch.from_numpy(np.frombuffer(raw, "<i4", n_rows * width, off).reshape(n_rows, width).copy())
        off += 4 * n_rows * width
        lp = torch.from_numpy(np.frombuffer(raw, "<f8", B * T * C, off).reshape(B, T, C).copy())
        off += 8 * B * T * C
        assert rc == 0, (l["name"], rc)
        try:
            bar, dist, worst = stage_a(x, lp, l["index"], n_rows, l["name"])
            got = stage_b(lp, l["sources"], l["index"], before, after, l["rec_at"], l["cap_len"], C, l["name"])
        except AssertionError as e:
            bad += 1
            print("MISMATCH %s: %s" % (l["name"], e))
            continue
        print("%-18s T %3d, n %2d, C %2d, cap_len %3d: bar %.3g, program - specification of lp %.3g, flags %s, records bit-equal"
              % (l["name"], T, B, C, l["cap_len"], bar, worst, "".join("-" if g is None else str(g.flag) for g in got)))
    assert off == len(raw)
    if not a.keep:
        shutil.rmtree(work)
    print("host check clean" if not bad else "host check FAILED: %d launches differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
