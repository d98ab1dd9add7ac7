// Stand-in of tatt_amd/csrc/common.h and of the HIP device environment for ONE kernel file compiled for the CPU (tools/words_host_check.py
// copies csrc/ctcwords.hip and csrc/ctc_f64.h beside this file, so that their #include "common.h" finds it): a work-group is a set of host
// threads, one per lane; a barrier is a pthread barrier; the data-parallel-primitive moves, readlane and ballot go through an array of the
// wave between two barriers of the wave's 64 threads; LDS maxima and minima are compare-and-swap loops; the dynamic LDS is one global
// array, poisoned before every work-group and checked beyond the launch's byte count after it.  Global memory is whatever the caller
// allocated: under -fsanitize=address,undefined every access of the kernel is checked against it.
#pragma once
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <functional>
#include <thread>
#include <vector>

#define TATT_HOST_STANDIN 1
#define TATT_API extern "C"
#define __global__
#define __device__
#define __shared__
#define __forceinline__ inline
#define __host__
#define __launch_bounds__(n)
#define LAUNCH_CHECK() 0

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
enum { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
extern size_t standin_lds_limit;                                     // what hipFuncSetAttribute allowed
static inline int hipFuncSetAttribute(const void*, int, int bytes) {
    standin_lds_limit = (size_t)bytes;
    return 0;
}
struct TattPerDevice { int unused; };
template <class F>
static inline void tatt_per_device(TattPerDevice&, F f) { f(); }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

extern thread_local dim3 threadIdx, blockIdx, blockDim;

#define STANDIN_LDS_BYTES (160 * 1024)
#define STANDIN_MAX_WAVES 16
struct StandinBlock {
    pthread_barrier_t all, wave[STANDIN_MAX_WAVES];
    int xi[STANDIN_MAX_WAVES][64];
    int any;
};
extern StandinBlock standin_block;

static inline void standin_wave_sync() { pthread_barrier_wait(&standin_block.wave[threadIdx.x >> 6]); }
static inline void __syncthreads() { pthread_barrier_wait(&standin_block.all); }
static inline int __syncthreads_or(int p) {
    if (p) __atomic_store_n(&standin_block.any, 1, __ATOMIC_SEQ_CST);
    __syncthreads();
    const int r = __atomic_load_n(&standin_block.any, __ATOMIC_SEQ_CST);
    __syncthreads();
    if (threadIdx.x == 0) standin_block.any = 0;
    __syncthreads();
    return r;
}

// update_dpp with the controls the CTC decoders use: row_shr:1 .. 15, row_shl:1 .. 15 (the suffix scan of ctcpat.hip), row_bcast:15,
// row_bcast:31; bound_ctrl off: a lane without a source, or in a row the row mask leaves out, keeps `old`
static inline int standin_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, row = l >> 4, i = l & 15;
    if (bank_mask != 0xf || bound_ctrl) abort();
    standin_block.xi[w][l] = src;
    standin_wave_sync();
    int from = -1;
    if (ctrl >= 0x111 && ctrl <= 0x11f) {
        if (i >= ctrl - 0x110) from = l - (ctrl - 0x110);
    } else if (ctrl >= 0x101 && ctrl <= 0x10f) {
        if (i + (ctrl - 0x100) <= 15) from = l + (ctrl - 0x100);
    } else if (ctrl == 0x142) {
        if (row >= 1) from = (row - 1) * 16 + 15;
    } else if (ctrl == 0x143) {
        if (row >= 2) from = 31;
    } else {
        abort();
    }
    const int r = from >= 0 && ((row_mask >> row) & 1) ? standin_block.xi[w][from] : old;
    standin_wave_sync();
    return r;
}
#define __builtin_amdgcn_update_dpp(old, src, ctrl, rm, bm, bc) standin_dpp((old), (src), (ctrl), (rm), (bm), (bc))
static inline int standin_readlane(int v, int k) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    standin_block.xi[w][l] = v;
    standin_wave_sync();
    const int r = standin_block.xi[w][k];
    standin_wave_sync();
    return r;
}
#define __builtin_amdgcn_readlane(v, k) standin_readlane((v), (k))
static inline unsigned long long __ballot(int p) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    standin_block.xi[w][l] = p != 0;
    standin_wave_sync();
    unsigned long long m = 0;
    for (int k = 0; k < 64; ++k) m |= (unsigned long long)(standin_block.xi[w][k] & 1) << k;
    standin_wave_sync();
    return m;
}
#define __builtin_amdgcn_sched_barrier(m) ((void)0)

static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
    }
    return old;
}
static inline unsigned atomicMin(unsigned* p, unsigned v) {
    unsigned old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
    }
    return old;
}

static inline long long __double_as_longlong(double v) {
    long long r;
    memcpy(&r, &v, 8);
    return r;
}
static inline double __longlong_as_double(long long v) {
    double r;
    memcpy(&r, &v, 8);
    return r;
}
static inline int __double2hiint(double v) { return (int)(__double_as_longlong(v) >> 32); }
static inline int __double2loint(double v) { return (int)(__double_as_longlong(v) & 0xffffffffll); }
static inline double __hiloint2double(int hi, int lo) {
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
static inline int __float_as_int(float v) {
    int r;
    memcpy(&r, &v, 4);
    return r;
}
static inline float __int_as_float(int v) {
    float r;
    memcpy(&r, &v, 4);
    return r;
}

// one work-group after the other, every lane a thread
void standin_launch(dim3 grid, dim3 block, size_t lds, const std::function<void()>& body);
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) standin_launch((grid), (block), (lds), [=] { kernel(__VA_ARGS__); })
