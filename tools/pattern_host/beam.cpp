// One of the two translation units of the stand-alone host check of pattern decoding (tools/pattern_host_check.py builds and runs it
// with -fsanitize=address,undefined): csrc/ctcbeam.hip compiled for the CPU.  Its directory holds tools/beam_lm_host/common.h as
// common.h (static LDS: `__shared__` becomes `static`) and tools/words_host/common.h as words_common.h; main.cpp, in a directory of its
// own with the plain stand-in as common.h (dynamic LDS), holds csrc/ctcpat.hip, the globals of the stand-in and the launcher.  The
// entries of this file have C linkage: main.cpp declares the two it calls.
#include "ctcbeam.hip"
