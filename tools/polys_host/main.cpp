// The check and the pixel function of tatt_poly_paste_u8 (csrc/poly_pixel.h) off the GPU: a stand-alone program for the sanitizers, driven
// by tools/polys_host_check.py.  It reads the item rows, the strip rows, the line buffer, the destination before the launch and the
// destination the specification expects from the files of the working directory, walks the kernel's grid (tile x item, 256 threads) and
// compares every byte.  Exit status 0 where no byte differs.
#define PLY_HD
#include "poly_pixel.h"

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

int main() {
    const auto rows = load<int>("rows.bin"), strips = load<int>("strips.bin");
    const auto src = load<unsigned char>("src.bin"), want = load<unsigned char>("want.bin");
    auto dst = load<unsigned char>("before.bin");
    const int n_items = (int)(rows.size() / PLY_DESC), n_strips = (int)(strips.size() / PLY_STRIP_DESC);
    long tiles = 0;
    for (int it = 0; it < n_items; ++it) {                           // the host entry's loop
        const int* d = rows.data() + (long)it * PLY_DESC;
        const int rc = ply_check(d, strips.data(), n_strips, (long)src.size(), (long)dst.size());
        if (rc) {
            printf("item %d refused with code %d\n", it, rc);
            return 1;
        }
        const long t = ply_tiles(d[5], d[6]);
        if (t > tiles) tiles = t;
    }
    long pixels = 0;
    for (int it = 0; it < n_items; ++it) {                           // the kernel's grid
        const int* d = rows.data() + (long)it * PLY_DESC;
        if (ply_check(d, strips.data(), n_strips, (long)src.size(), (long)dst.size()) != 0) continue;
        for (long t = 0; t < tiles; ++t)
            for (int tid = 0; tid < 256; ++tid) {
                int i, j;
                if (!ply_place(t, tid, d[5], d[6], &i, &j)) continue;
                ply_pixel(d, strips.data() + (long)d[9] * PLY_STRIP_DESC, src.data() + d[0], i, j, dst.data() + d[4] + i * (long)d[7] + j * 3L);
                ++pixels;
            }
    }
    long bad = 0;
    for (size_t k = 0; k < dst.size(); ++k) bad += dst[k] != want[k];
    printf("%d items, %d strips, %ld pixels: %ld of %zu bytes differ from the specification\n", n_items, n_strips, pixels, bad, dst.size());
    return bad != 0;
}
