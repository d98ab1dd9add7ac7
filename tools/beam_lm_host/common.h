// Stand-in of tatt_amd/csrc/common.h for csrc/ctcbeam.hip compiled for the CPU (tools/beam_lm_host_check.py copies the kernel file,
// csrc/ctc_f64.h and tools/words_host/common.h -- the thread-per-lane stand-in of the wave, as words_common.h -- beside this file).  What
// the beam kernel needs beyond that stand-in: its LDS is STATIC, not dynamic, so `__shared__` becomes `static` (one copy per
// instantiation, shared by the lane threads of a work-group; work-groups run one after the other), plus two more wave intrinsics.
#pragma once
#include "words_common.h"

#undef __shared__
#define __shared__ static
#define __host__
static inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
#define __builtin_amdgcn_readfirstlane(v) standin_readlane((v), 0)
