"""The polygon paste and the warp off the GPU: the checks and the pixel functions of tatt_poly_paste_u8 and tatt_warp_u8
(csrc/warp_pixel.h, `__host__ __device__`: the very text the kernels run) compiled with tools/polys_host/main.cpp into a STAND-ALONE
program under -fsanitize=address,undefined and run in two passes: over the items of tests/test_polys_device_gpu.py (N = 2, 4, 5 and 8;
targets of 1, tile - 1, tile and tile + 1 rows and columns; feather 0, 1 and 5; scale 1 and 2; lines and targets at non-zero offsets with
wide pitches) against arrays the specification (`tatt_amd.polys.poly_paste_host`) writes, and over the rows of tests/
test_quads_device_gpu.py (identity, rotated and perspective matrices; the same target sizes; both modes; feather 0, 1 and 5) against
arrays `tatt_amd.quads.warp_u8_host` writes.  Nothing is loaded into this process.  It is a check for the BUILD machine (CPUs, no GPU); it
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
    from tests.test_quads_device_gpu import warp_items, warp_layout, warp_wants

    def expected(before, want, rects):
        full = before.copy()
        for w, (o, dp, oh, ow) in zip(want, rects):
            np.lib.stride_tricks.as_strided(full[o:], (oh, ow, 3), (dp, 3, 1))[...] = w
        return full
    items = paste_items()
    rows, strips, sbuf, before, rects = paste_layout(items)
    full = expected(before, paste_wants(items, before, rects)[0], rects)
    items = warp_items()
    wrows, wsbuf, wbefore, wrects = warp_layout(items)
    wfull = expected(wbefore, warp_wants(items, wbefore, wrects)[0], wrects)
    work = a.keep or tempfile.mkdtemp(prefix="polys_host_")
    os.makedirs(work, exist_ok=True)
    try:
        for name, arr in (("rows", rows), ("strips", strips), ("src", sbuf), ("before", before), ("want", full), ("warp_rows", wrows),
                          ("warp_src", wsbuf), ("warp_before", wbefore), ("warp_want", wfull)):
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
