// The checks and the pixel functions of tatt_poly_paste_u8 and of tatt_warp_u8 (csrc/warp_pixel.h) off the GPU: a stand-alone program for
// the sanitizers, driven by tools/polys_host_check.py.  Two passes.  Each reads its rows (the polygon pass its strip rows too), the source
// buffer, the destination before the launch and the destination the specification expects from the files of the working directory, walks
// its kernel's grid (tile x item, 256 threads) and compares every byte.  Exit status 0 where no byte differs.
#define WARP_HD
#include "warp_pixel.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

template <class T>
static std::vector<T> load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v(n / sizeof(T));
    if (fread(v.data(), 1, n, f) != (size_t)n) exit(2);
    fclose(f);
    return v;
}

// one entry and its kernel: check(d) the row check, pixel(d, i, j, q) the pixel function on destination `dst`; d = rows + item * desc
template <class Check, class Pixel>
static bool pass(const char* what, const std::vector<int>& rows, int desc, std::vector<unsigned char>& dst,
                 const std::vector<unsigned char>& want, Check check, Pixel pixel) {
    const int n_items = (int)(rows.size() / desc);
    long tiles = 0;
    for (int it = 0; it < n_items; ++it) {                           // the host entry's loop
        const int* d = rows.data() + (long)it * desc;
        const int rc = check(d);
        if (rc) {
            printf("%s: item %d refused with code %d\n", what, it, rc);
            return false;
        }
        const long t = warp_tiles(d[5], d[6]);
        if (t > tiles) tiles = t;
    }
    long pixels = 0;
    for (int it = 0; it < n_items; ++it) {                           // the kernel's grid
        const int* d = rows.data() + (long)it * desc;
        if (check(d) != 0) continue;
        for (long t = 0; t < tiles; ++t)
            for (int tid = 0; tid < 256; ++tid) {
                int i, j;
                if (!warp_place(t, tid, d[5], d[6], &i, &j)) continue;
                pixel(d, i, j, dst.data() + d[4] + i * (long)d[7] + j * 3L);
                ++pixels;
            }
    }
    long bad = 0;
    for (size_t k = 0; k < dst.size(); ++k) bad += dst[k] != want[k];
    printf("%s: %d items, %ld pixels: %ld of %zu bytes differ from the specification\n", what, n_items, pixels, bad, dst.size());
    return bad == 0;
}

int main() {
    const auto rows = load<int>("rows.bin"), strips = load<int>("strips.bin");
    const auto src = load<unsigned char>("src.bin"), want = load<unsigned char>("want.bin");
    auto dst = load<unsigned char>("before.bin");
    const int n_strips = (int)(strips.size() / PLY_STRIP_DESC);
    const long sb = (long)src.size(), db = (long)dst.size();
    bool ok = pass(
        "tatt_poly_paste_u8", rows, PLY_DESC, dst, want, [&](const int* d) { return ply_check(d, strips.data(), n_strips, sb, db); },
        [&](const int* d, int i, int j, unsigned char* q) {
            ply_pixel(d, strips.data() + (long)d[9] * PLY_STRIP_DESC, src.data() + d[0], i, j, q);
        });
    const auto wrows = load<int>("warp_rows.bin");
    const auto wsrc = load<unsigned char>("warp_src.bin"), wwant = load<unsigned char>("warp_want.bin");
    auto wdst = load<unsigned char>("warp_before.bin");
    const long wsb = (long)wsrc.size(), wdb = (long)wdst.size();
    ok &= pass(
        "tatt_warp_u8", wrows, WRP_DESC, wdst, wwant, [&](const int* d) { return wrp_check(d, wsb, wdb); },
        [&](const int* d, int i, int j, unsigned char* q) { wrp_pixel(d, wsrc.data() + d[0], i, j, q); });
    return ok ? 0 : 1;
}
