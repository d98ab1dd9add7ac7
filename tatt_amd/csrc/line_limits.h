// The limits of tatt_line_windows (lines.hip) and tatt_scene_windows (scene.hip), reported by tatt_line_limits: ONE set, so that one host
// fallback decides for both entries.
#pragma once
#include "pil_resample.h"         // col_ksize

#define LIN_THREADS 256
#define LIN_MAX_ROWS 256               // source rows / columns the resampling passes take
#define LIN_MAX_COLS 16384
#define LIN_MAX_WL 4096                // widest line at the window height
#define LIN_MAX_H 64                   // largest window
#define LIN_MAX_W 256
#define LIN_MAX_INTER 65536            // bytes of the horizontal pass's result (H_src * w * 3)
#define LIN_MAX_TABLE 32768            // bytes of the horizontal coefficient rows (w * ksize * 4)
#define LIN_LDS 126976                 // most dynamic LDS of a launch

// the geometry both entries take: an H_src x W_src source, the h x w window at column x0 of its wl columns at height h
static __host__ __device__ inline bool lin_takes(int hs, int ws, int h, int wl, int x0, int w) {
    if (hs < 1 || ws < 1 || h < 1 || w < 1 || h > LIN_MAX_H || w > LIN_MAX_W || wl < w || wl > LIN_MAX_WL) return false;
    if (x0 < 0 || x0 > wl - w || hs > LIN_MAX_ROWS || ws > LIN_MAX_COLS) return false;
    return ws == wl || ((long)hs * w * 3 <= LIN_MAX_INTER && (long)w * col_ksize(ws, wl) * 4 <= LIN_MAX_TABLE);
}
