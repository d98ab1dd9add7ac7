"""The polygon paste off the GPU: the check and the pixel function of tatt_poly_paste_u8 (csrc/poly_pixel.h, `__host__ __device__`: the
very text the kernel runs) compiled with tools/polys_host/main.cpp into a STAND-ALONE program under -fsanitize=address,undefined and run
over the items of tests/test_polys_device_gpu.py (N = 2, 4, 5 and 8; targets of 1, tile - 1, tile and tile + 1 rows and columns; feather
0, 1 and 5; scale 1 and 2; lines and targets at non-zero offsets with wide pitches) against arrays the specification
(`tatt_amd.polys.poly_paste_host`) writes.  Nothing is loaded into this process.  It is a check for the BUILD machine (CPUs, no GPU); it
is not run on a GPU machine, and it stops where LD_PRELOAD is set: a sanitized program must be the first thing loaded, and the tool
leaves that setting as it is.

    python tools/polys_host_check.py [--keep DIR]

Exit status 0 and "host check clean" where no byte differs and the sanitizers reported nothing."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run here, and keep the files")
    a = ap.parse_args()
    if os.environ.get("LD_PRELOAD"):
        print("host check not run: LD_PRELOAD is set here.  The check is meant for the build machine, which has no GPU and preloads "
              "nothing; it leaves the setting as it is.")
        return 2
    from tests.test_polys_device_gpu import paste_items, paste_layout, paste_wants
    items = paste_items()
    rows, strips, sbuf, before, rects = paste_layout(items)
    want, _ = paste_wants(items, before, rects)
    full = before.copy()
    for w, (o, dp, oh, ow) in zip(want, rects):
        np.lib.stride_tricks.as_strided(full[o:], (oh, ow, 3), (dp, 3, 1))[...] = w
    work = a.keep or tempfile.mkdtemp(prefix="polys_host_")
    os.makedirs(work, exist_ok=True)
    try:
        for name, arr in (("rows", rows), ("strips", strips), ("src", sbuf), ("before", before), ("want", full)):
            arr.tofile(os.path.join(work, name + ".bin"))
        cxx = os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++")
        exe = os.path.join(work, "polys_host")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "tatt_amd", "csrc"), os.path.join(ROOT, "tools", "polys_host", "main.cpp"), "-o", exe],
                       check=True)
        r = subprocess.run([exe], cwd=work, capture_output=True, text=True, timeout=600)
        print(r.stdout.strip())
        if r.returncode != 0 or r.stderr.strip():
            print(r.stderr.strip())
            print("host check FAILED (exit status %d)" % r.returncode)
            return 1
        print("host check clean")
        return 0
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
