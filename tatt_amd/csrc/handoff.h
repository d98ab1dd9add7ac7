// The ONE in-flight hand-off between work-groups of a launch (device only).  Used by the persistent query-GRU chains (gru.hip), the
// recognisers' LSTM chain (infer.hip) and the STN-head launches (stnhead.hip); each of them says only WHAT crosses work-groups and how
// its flags are laid out, the protocol is here:
//
//   producer   every byte that another work-group will read is stored with 16-byte `sc1` (write-through) stores (st16_sc1);
//              the waves that stored -- and, in the chains, ONLY those: the other waves have next step's loads in flight, which a drain
//              would wait for -- run handoff_drain() (s_waitcnt vmcnt(0));
//              handoff_post(): a work-group barrier, then ONE relaxed agent-scope store of the work-group's flag word by thread 0.
//   consumer   HANDOFF_WAIT: wave 0 polls the flag words it depends on with relaxed agent-scope loads (one or two words per lane,
//              a ballot, s_sleep 1 between trips), then a work-group barrier that every wave joins; only after it are the handed-off
//              bytes loaded, every one of them with an `sc1` load (ld16_sc1: never from this CU's L1).
//   expiry     every poll is bounded by the wall clock, looked at every 64th trip.  When HANDOFF_SPIN_TICKS have passed, lane 0 sets the
//              work-group's `dead` word in LDS (later waits of the launch return at once), stores 1 to the launch's error word and ORs
//              the family's code into the device's sticky word (common.h); the launch then runs on WITHOUT waiting -- its results are
//              garbage but it ends -- and the host reports it when it next synchronises (functional.sync_check).
//   residency  a work-group waits for others of the SAME launch, so all the work-groups that wait on one another must be on the chip
//              together: the entry points refuse grids beyond the capacity they asked the runtime for; what a capacity cannot see (a
//              CU mask, CUs held by other launches) is what the bound is for.
//
// This is the first row of the hand-off table of MI355X_MICROARCH.md ("ONE lane of each storing workgroup, for ALL that workgroup's
// stores: an sc1 flag store" | "an sc1 load poll of that flag" | "the other waves load after a workgroup barrier that wave then joins" |
// hipMalloc, one work-group per CU | 16-byte sc1 stores | 16-byte sc1 loads), with consumer conditions (1) to (4) of that guide.
#pragma once
#include "common.h"

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// 2 s of the 100 MHz wall clock: far beyond any stall another launch (a collective waiting for a late rank) can cause
#define HANDOFF_SPIN_TICKS 200000000L

// 16-byte write-through store / L1-bypassing load at base + off bytes, through a buffer descriptor of `range` bytes (base and range
// wave-uniform: the descriptor stays in SGPRs; an access beyond the range is dropped / reads zero)
__device__ __forceinline__ void st16_sc1(void* base, int range, int off, const void* v16) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, range, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4_t*>(v16), rs, off, 0, 16 /* sc1: write-through */);
}
__device__ __forceinline__ u32x4_t ld16_sc1(const void* base, int range, int off) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, range, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16 /* sc1: not from this CU's L1 */);
}

// the storing waves' wait for their stores.  The CALLER decides which threads run it (see `producer` above): not part of handoff_post
__device__ __forceinline__ void handoff_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// called by every thread, after the storing waves' handoff_drain()
__device__ __forceinline__ void handoff_post(unsigned* flag, unsigned value) {
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// HANDOFF_WAIT: flags[0 .. n-1] have all reached `value`.  A statement for every thread of the work-group; it ends with a barrier.
//   polls, lane    this thread belongs to wave 0 / its lane there, as the kernel already has them (`wave == 0`, `t & 63`)
//   per_lane       1 or 2 flag words per lane: n <= 64 * per_lane; lanes beyond n count as published
//   dead           the work-group's `dead` word in LDS (an lvalue), zeroed by the kernel before its first wait
//   err_word, sticky, code     what an expiry raises (above)
// The compare is wrap-safe (the STN head's flags are epoch-stamped and never reset); the chains' flags count steps from 0 up to
// T < 2^31, for which it equals the plain `f < value`.
// A macro, not a function: as an inlined function the loop is simplified on its own before it meets the kernel's step loop, which
// changes register allocation and scheduling THROUGHOUT the chain kernels; expanded in place they compile as they did with the loop
// written out (profiles/handoff_isa_diff.txt).
#define HANDOFF_WAIT(polls, lane, per_lane, flags, n, value, dead, err_word, sticky, code)                                                \
    {                                                                                                                                     \
        static_assert((per_lane) == 1 || (per_lane) == 2, "one or two flag words per lane of wave 0");                                    \
        if ((polls) && !(dead)) {                                                                                                         \
            const long t0_ = wall_clock64();                                                                                              \
            int it_ = 0;                                                                                                                  \
            for (;;) {                                                                                                                    \
                const unsigned f0_ = (lane) < (n) ? __hip_atomic_load((flags) + (lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (value); \
                const unsigned f1_ = (per_lane) == 2 && (lane) + 64 < (n) ? __hip_atomic_load((flags) + (lane) + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (value); \
                if (__builtin_amdgcn_ballot_w64((int)(f0_ - (value)) < 0 || (int)(f1_ - (value)) < 0) == 0) break;                        \
                __builtin_amdgcn_s_sleep(1);                                                                                              \
                if ((++it_ & 63) == 0 && wall_clock64() - t0_ > HANDOFF_SPIN_TICKS) {                                                     \
                    if ((lane) == 0) { (dead) = 1; __hip_atomic_store(err_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); tatt_raise_sticky(sticky, code); } \
                    break;                                                                                                                \
                }                                                                                                                         \
            }                                                                                                                             \
        }                                                                                                                                 \
        __syncthreads();                                                                                                                  \
    }
