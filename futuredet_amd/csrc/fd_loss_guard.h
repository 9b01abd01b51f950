// The skip-and-count rule of the fused CenterHead loss (fd_loss.hip), as plain arithmetic that compiles for the host too: a CPU
// test drives it through a small stand-alone program, because a wrong guard cannot be tested on a device without faulting it.
//
//   mask == 0                                   -> kLossSkip : contributes nothing; its ind / cat are never used as an index
//   mask != 0, ind in [0, HW), cat in [0, C)    -> kLossTake
//   mask != 0, anything else                    -> kLossBad  : contributes nothing and is counted in the status word (torch would
//                                                              device-assert in gather)
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

enum { kLossSkip = 0, kLossTake = 1, kLossBad = 2 };

__host__ __device__ inline int fd_loss_entry_kind(uint8_t mask, int64_t ind, int64_t cat, int64_t hw, int channels) {
    if (mask == 0) return kLossSkip;
    if (ind < 0 || ind >= hw || cat < 0 || cat >= (int64_t)channels) return kLossBad;
    return kLossTake;
}

// Element of a [B, channels, HW] map that entry (b, ch, ind) names, or -1 when any of the three is out of range: the last line of
// defence in front of every gather of the kernels (the callers only pass entries of kind kLossTake).
__host__ __device__ inline int64_t fd_loss_cell(int b, int B, int ch, int channels, int64_t ind, int64_t hw) {
    if (b < 0 || b >= B || ch < 0 || ch >= channels || ind < 0 || ind >= hw) return -1;
    return ((int64_t)b * channels + ch) * hw + ind;
}
