// The per-pair arithmetic of every TransE distance kernel (k_transe.hip: te_tile and the ranker's target distance;
// k_transe_mine.hip: the whole-graph miner).  One definition, so all of them produce the same bits.
#pragma once
#include "common.h"

namespace gv {

constexpr int TE_TQ = 64, TE_TE = 64;   // queries x entities per workgroup tile: 256 threads, 4 x 4 pairs a lane

// one column of ||a - b||_p into the pair's single accumulator (p = 2: the caller takes sqrtf at the end)
__device__ __forceinline__ float te_pair_term(float acc, float a, float b, int p) {
    const float d = a - b;
    return p == 1 ? acc + fabsf(d) : fmaf(d, d, acc);
}

}  // namespace gv
