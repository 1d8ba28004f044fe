// Riders: small launches of the forward head and of the backward's gradient finishers whose inputs do not depend on the product
// beside them, as bodies that take (block index, block count) instead of blockIdx / gridDim.  The stand-alone kernels (k_rng_fill,
// k_pack_weight, k_kl_mix, k_prior_sample_fwd) call the same bodies, and so do the extra workgroups of k_gemm_f32_riders
// (k_gemm.hip): every expression and every order is shared, so a value does not depend on which launch wrote it.  The two slice-sum
// finishers (k_kl_bwd_mix_final, k_colsum_final_wide) keep their 1024-thread launches; their rider bodies are 256-thread
// workgroups that form the same 64 slice-group sums with the same function and add them in the same order (common.h:
// slice_group_sum, slice_groups_total), and share the store expressions below.
// Rules of a rider: no atomics, no waiting of one workgroup on another; it reads nothing the product writes and writes nothing
// the product reads (gv_gemm_f32_riders / _fin refuse overlapping buffers on the host).  LDS and barriers: only inside ONE rider
// workgroup -- the branch that selects a rider is block-uniform, so a __syncthreads() in a body is reached by all 256 threads --
// and only through the 64 x 16 float scratch that the riders kernel hands to rider_body.
#pragma once

#include "common.h"

namespace gv {

// ---- counter-based RNG: every random draw of one forward pass ---------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): key = the 64-bit seed, counter = (group, stream, tick_lo, tick_hi); one call
// yields the 4 outputs of elements 4*group .. 4*group+3 of a job.  `tick` is a device-side step counter (state[1]),
// so a captured hipGraph draws fresh numbers on every replay; `stream` separates the jobs of one tick.
//   kind 0: keep mask, byte = (u32 >= floor(p_drop * 2^32))            (nn.Dropout's Bernoulli(1-p) decision)
//   kind 1: standard normals by Box-Muller, (u1, u2) = ((x0 + 1) * 2^-32, x1 * 2^-32)  (torch.randn_like)
struct RngJobs {
    void* ptr[GV_RNG_MAX_JOBS];
    long long n[GV_RNG_MAX_JOBS];
    long long group0[GV_RNG_MAX_JOBS + 1];     // prefix of ceil(n/4): job j owns global groups [group0[j], group0[j+1])
    int kind[GV_RNG_MAX_JOBS];
    uint32_t thresh[GV_RNG_MAX_JOBS];
    uint32_t stream[GV_RNG_MAX_JOBS];
    int n_jobs;
};

__device__ __forceinline__ void rng_fill_body(const uint64_t* state, const RngJobs& jobs, long long bid, long long nblk) {
    const uint64_t seed = state[0], tick = state[1];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), t0 = (uint32_t)tick, t1 = (uint32_t)(tick >> 32);
    const long long total = jobs.group0[jobs.n_jobs];
    for (long long gg = bid * 256 + threadIdx.x; gg < total; gg += nblk * 256) {
        int j = 0;
#pragma unroll
        for (int q = 1; q < GV_RNG_MAX_JOBS; ++q)
            if (q < jobs.n_jobs && gg >= jobs.group0[q]) j = q;
        const long long grp = gg - jobs.group0[j];
        const uint4 x = philox4x32_10(k0, k1, (uint32_t)grp, jobs.stream[j], t0, t1);
        const long long e0 = grp * 4, left = jobs.n[j] - e0;
        if (jobs.kind[j] == 0) {
            const uint32_t th = jobs.thresh[j];
            uint8_t* o = (uint8_t*)jobs.ptr[j] + e0;
            const uchar4 b = make_uchar4(x.x >= th, x.y >= th, x.z >= th, x.w >= th);
            if (left >= 4) {
                *reinterpret_cast<uchar4*>(o) = b;
            } else {
                o[0] = b.x;
                if (left > 1) o[1] = b.y;
                if (left > 2) o[2] = b.z;
            }
        } else {
            // hardware transcendentals: v_log_f32 (base 2), v_sin/v_cos_f32 (argument in revolutions) -- ~1e-6 absolute
            // on the result, far inside what noise needs; the precise libm sincosf tripled this kernel's time
            const float s = 2.3283064365386963e-10f;       // 2^-32
            const float r0 = sqrtf(-1.3862943611198906f * __log2f(((float)x.x + 1.f) * s));    // -2 ln u = -2 ln2 log2 u
            const float r1 = sqrtf(-1.3862943611198906f * __log2f(((float)x.z + 1.f) * s));
            const float a0 = (float)x.y * s, a1 = (float)x.w * s;                                 // revolutions in [0, 1]
            const float s0 = __builtin_amdgcn_sinf(a0), c0 = __builtin_amdgcn_cosf(a0);
            const float s1 = __builtin_amdgcn_sinf(a1), c1 = __builtin_amdgcn_cosf(a1);
            const float4 nrm = make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
            float* o = (float*)jobs.ptr[j] + e0;
            if (left >= 4) {
                *reinterpret_cast<float4*>(o) = nrm;
            } else {
                o[0] = nrm.x;
                if (left > 1) o[1] = nrm.y;
                if (left > 2) o[2] = nrm.z;
            }
        }
    }
}

// ---- lane-packed bdd relation weights: row layout [R][nb*P*Q] -> lane-packed layout for (BPL, ownership); one thread per float4
__device__ __forceinline__ void pack_weight_body(const float* w, float* packed, int num_rels, int nb, int pq, int bpl, int adj,
                                                 int bid, int nblk) {
    const int L = nb / bpl, nq = bpl * pq / 4, quads = L * nq;     // float4 per relation row
    const int total = num_rels * quads;
    for (int i = bid * 256 + threadIdx.x; i < total; i += nblk * 256) {
        const int r = i / quads, rem = i - r * quads;
        const int l = rem % L, jq = rem / L;               // quad jq of lane l's weight list
        const int f = 4 * jq, sb = f / pq, within = f - sb * pq;
        const int block = adj ? l * bpl + sb : l + sb * L;
        reinterpret_cast<float4*>(packed)[i] =
            *reinterpret_cast<const float4*>(w + (size_t)r * nb * pq + (size_t)block * pq + within);
    }
}

// host side (k_bdd.hip): (bpl, adj) of the packed layout for one launch kind; false where no lane-packed kernel exists
bool pack_job_plan(int num_bases, int blk_in, int blk_out, bool transpose_w, int* bpl, int* adj);

// ---- the KL term's mixture table: mix[3][k*h] = (mu_j, 1/(2 v_j), log sqrt v_j + log sqrt 2pi) from z_pre (2k, h)
constexpr float LOG_SQRT_2PI = 0.9189385332046727f;

__device__ __forceinline__ float softplus_t(float x) { return x > 20.f ? x : log1pf(expf(x)); }

__device__ __forceinline__ void kl_mix_body(const float* z_pre, int k, int h, float* mix, int bid, int nblk) {
    const int total = k * h;
    for (int i = bid * 256 + threadIdx.x; i < total; i += nblk * 256) {
        const float v = softplus_t(z_pre[total + i]) + 1e-8f;
        mix[i] = z_pre[i];
        mix[total + i] = 1.f / (2.f * v);
        mix[2 * total + i] = logf(sqrtf(v)) + LOG_SQRT_2PI;
    }
}

// ---- prior samples of get_mmd: z_pri[i] = mu[i % k] + eps[i] * sqrt(softplus(raw[i % k]) + 1e-8)   (z_pre = [mu; raw], (2k, h))
__device__ __forceinline__ void prior_sample_body(const float* z_pre, const float* eps, float* out, int s, int k, int h, int bid, int nblk) {
    const int total = s * h;
    for (int i = bid * 256 + threadIdx.x; i < total; i += nblk * 256) {
        const int r = i / h, c = i - r * h, j = r % k;
        const float v = softplus_t(z_pre[(size_t)(k + j) * h + c]) + 1e-8f;
        out[i] = z_pre[(size_t)j * h + c] + eps[i] * sqrtf(v);
    }
}

// ---- the KL backward's finisher: column i of the slice sums -> z_pre's gradient (chained through v_j = softplus(raw) + 1e-8 in
// the second half) or, behind the 2 k h mixture columns, the bias gradient of the layer that made h2 (no factor, no chain)
__device__ __forceinline__ void kl_mix_final_store(float acc, int i, int kh, const float* z_pre, const float* gkl, float gscale,
                                                   float* g_zpre, int accumulate, int64_t n, const int* rows_dev, float* g_bias,
                                                   int accumulate_bias) {
    if (i >= 2 * kh) {
        g_bias[i - 2 * kh] = accumulate_bias ? g_bias[i - 2 * kh] + acc : acc;
        return;
    }
    const float cg = gscale * (gkl ? *gkl : 1.f) / (float)(rows_dev ? (int64_t)*rows_dev : n);
    if (i >= kh) {  // chain through v_j = softplus(raw) + 1e-8
        const float raw = z_pre[i];
        acc *= raw > 20.f ? 1.f : 1.f / (1.f + expf(-raw));
    }
    g_zpre[i] = accumulate ? g_zpre[i] + cg * acc : cg * acc;
}

struct KlFinJob {
    const float* part;     // [nsl][2 k h (+ 2 h)]
    const float* z_pre;
    const float* gkl;
    float gscale;
    float* g_zpre;
    float* g_bias;         // or NULL
    long long n;
    int accumulate, accumulate_bias, h, k, nsl;
};

__device__ __forceinline__ void kl_mix_final_body(const KlFinJob& j, int bid, float (*sm)[16]) {
    const int kh = j.k * j.h, total = 2 * kh + (j.g_bias ? 2 * j.h : 0);
    const int i = bid * 16 + (threadIdx.x & 15);
    const float acc = sum_slices_16x64_wg256(j.part, total, j.nsl, i, sm);
    if ((threadIdx.x >> 4) != 0 || i >= total) return;
    kl_mix_final_store(acc, i, kh, j.z_pre, j.gkl, j.gscale, j.g_zpre, j.accumulate, j.n, nullptr, j.g_bias, j.accumulate_bias);
}

// ---- a bias gradient from the column-sum partials of an epilogue backward: out[c] (+)= sum over the slices
struct ColsumJob {
    const float* part;     // [nsl][n]
    float* out;
    int n, nsl, accumulate;
};

__device__ __forceinline__ void colsum_final_store(float acc, int c, float* out, int accumulate) {
    out[c] = accumulate ? out[c] + acc : acc;
}

__device__ __forceinline__ void colsum_final_body(const ColsumJob& j, int bid, float (*sm)[16]) {
    const int c = bid * 16 + (threadIdx.x & 15);
    const float acc = sum_slices_16x64_wg256(j.part, j.n, j.nsl, c, sm);
    if ((threadIdx.x >> 4) == 0 && c < j.n) colsum_final_store(acc, c, j.out, j.accumulate);
}

// ---- what one launch carries: the jobs, and per rider kind the prefix of its workgroup count --------------------
struct PackJob {
    const float* w;
    float* packed;
    float* packed2;        // the second layout of the same weights (a layer's backward-x launch), or NULL
    int num_rels, nb, pq, bpl, adj, bpl2, adj2;
    int blocks;            // workgroups per layout
};

struct MixJob {
    const float* z_pre;
    float* mix;
    int k, h;
};

struct PriorJob {
    const float* z_pre;
    const float* eps;
    float* out;
    int s, k, h;
};

struct RiderSet {
    const uint64_t* rng_state;
    RngJobs rng;
    PackJob pack;
    MixJob mix;
    PriorJob prior;
    KlFinJob klfin;
    ColsumJob colsum;
    // rider block b belongs to: RNG [first[0], first[1]), pack [first[1], first[2]), mix [first[2], first[3]), prior samples
    // [first[3], first[4]), KL finisher [first[4], first[5]), column sums [first[5], first[6])
    int first[7];
};

// rider block `b` of `n` (n >= first[6]: the blocks behind first[6] only pad the count and leave at once); block-uniform branches.
// `sm`: the workgroup's 64 x 16 float scratch (the slice-sum finishers)
__device__ __forceinline__ void rider_body(const RiderSet& rs, int b, int n, float (*sm)[16]) {
    (void)n;
    if (b < rs.first[1]) {
        rng_fill_body(rs.rng_state, rs.rng, b, rs.first[1]);
    } else if (b < rs.first[2]) {
        const int i = b - rs.first[1], second = i >= rs.pack.blocks;
        const PackJob& pj = rs.pack;
        pack_weight_body(pj.w, second ? pj.packed2 : pj.packed, pj.num_rels, pj.nb, pj.pq, second ? pj.bpl2 : pj.bpl,
                         second ? pj.adj2 : pj.adj, second ? i - pj.blocks : i, pj.blocks);
    } else if (b < rs.first[3]) {
        kl_mix_body(rs.mix.z_pre, rs.mix.k, rs.mix.h, rs.mix.mix, b - rs.first[2], rs.first[3] - rs.first[2]);
    } else if (b < rs.first[4]) {
        prior_sample_body(rs.prior.z_pre, rs.prior.eps, rs.prior.out, rs.prior.s, rs.prior.k, rs.prior.h, b - rs.first[3],
                          rs.first[4] - rs.first[3]);
    } else if (b < rs.first[5]) {
        kl_mix_final_body(rs.klfin, b - rs.first[4], sm);
    } else if (b < rs.first[6]) {
        colsum_final_body(rs.colsum, b - rs.first[5], sm);
    }
}

}  // namespace gv
