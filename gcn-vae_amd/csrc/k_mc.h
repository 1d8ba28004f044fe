// The one sigmoid of the Monte-Carlo posterior-predictive scorers (k_gemm.hip: gv_rank_scores_mc, gv_topk_scores_mc,
// gv_pair_prob_std_mc; k_mine.hip: gv_mine_scores_typed_mc).  One definition for both translation units, so a pair's probability
// is bit-identical whichever of them computed it.
#pragma once
#include "common.h"

namespace gv {

// sig(x) = 1 / (1 + exp(-x)), as v_rcp_f32(1.0f + __expf(-x)): two quarter-rate instructions, no IEEE divide sequence.  The ONE form
// every pass and entry point of the MC scorers uses, so a target's probability is bit-identical wherever it is recomputed.
// +inf -> 1, -inf -> 0 (exp overflows to +inf, whose reciprocal is +0), NaN -> NaN: a NaN in any sample makes pbar NaN.
__device__ __forceinline__ float mc_sig(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

}  // namespace gv
