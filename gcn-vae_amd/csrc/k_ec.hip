// Entity classification (kgvae/entity_classify.py): the basis-decomposed integer-id input layer without the (R, N, h) weight, and
// the softmax / cross-entropy head.  Every sum here has a fixed order: no float atomics, the same bits on every run.
//
// Basis rows.  A "run" is one distinct (id, relation) pair among the edges (the plan, ops.basis_select_plan, sorts the runs by id,
// then relation).  Every edge of a run carries the same message -- row id of W_r = sum_b comp[r, b] V_b -- so the forward makes
// that row once per run:
//     msg[k, :] = sum_b comp[rel_k, b] V[b, id_k, :]
// and the existing 1x1-block aggregation sums the runs' rows into the destinations.  Backward, with S[k, :] = sum over the run's
// edges of norm_e g[dst_e] (the same aggregation over the transposed incidence):
//     dV[b, id, :]  = sum over the runs k of id  comp[rel_k, b] S[k, :]        one thread per (id, b, column)
//     Q[k, b]       = V[b, id_k, :] . S[k, :]                                  written in relation order
//     dcomp[r, b]   = sum over the runs k of r  Q[k, b]                        one workgroup per relation, fixed-order tree
// V offsets are 64-bit: nb * rows * h passes 2^31 at the AM size.
#include "common.h"

namespace gv {

#define GV_ST ((hipStream_t)stream)

static inline int ec_grid(int64_t n, int per_block) {
    int64_t b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

constexpr int EC_COMP_LDS_MAX = 64 * 1024;   // bytes of comp staged in LDS (AM: 266 x 40 floats = 42.6 KB); more is read from L2

template <bool LDS>
__global__ __launch_bounds__(256) void k_ec_basis_rows_fwd(const float* __restrict__ v, const float* __restrict__ comp,
                                                           const int32_t* __restrict__ run_id, const int32_t* __restrict__ run_rel,
                                                           int64_t n_runs, int h, int nb, int num_rels, int64_t rows,
                                                           float* __restrict__ msg) {
    extern __shared__ float comp_s[];
    const float* cp = comp;
    if (LDS) {
        for (int i = threadIdx.x; i < num_rels * nb; i += blockDim.x) comp_s[i] = comp[i];
        __syncthreads();
        cp = comp_s;
    }
    const int64_t total = n_runs * h, plane = rows * h;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = t / h;
        const int c = (int)(t - k * h);
        const float* vp = v + (int64_t)run_id[k] * h + c;
        const float* cr = cp + (int64_t)run_rel[k] * nb;
        float acc = 0.f;
        for (int b = 0; b < nb; ++b) acc = fmaf(cr[b], vp[b * plane], acc);
        msg[t] = acc;
    }
}

// dV for the ids that occur (the runs of group g are run_ptr[g] .. run_ptr[g+1]); rows of other ids are not touched
__global__ __launch_bounds__(256) void k_ec_basis_dv(const float* __restrict__ s, const float* __restrict__ comp,
                                                     const int32_t* __restrict__ run_id, const int32_t* __restrict__ run_rel,
                                                     const int64_t* __restrict__ run_ptr, int64_t n_groups, int h, int nb,
                                                     int64_t rows, int accumulate, float* __restrict__ dv) {
    const int64_t per = (int64_t)nb * h, total = n_groups * per, plane = rows * h;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = t / per;
        const int rem = (int)(t - g * per);
        const int b = rem / h, c = rem - b * h;
        const int64_t k0 = run_ptr[g], k1 = run_ptr[g + 1];
        float acc = 0.f;
        for (int64_t k = k0; k < k1; ++k) acc = fmaf(comp[(int64_t)run_rel[k] * nb + b], s[k * h + c], acc);
        float* o = dv + b * plane + (int64_t)run_id[k0] * h + c;
        *o = accumulate ? *o + acc : acc;
    }
}

// Q[q_pos[k], b] = V[b, id_k, :] . S[k, :]
__global__ __launch_bounds__(256) void k_ec_basis_q(const float* __restrict__ v, const float* __restrict__ s,
                                                    const int32_t* __restrict__ run_id, const int64_t* __restrict__ q_pos,
                                                    int64_t n_runs, int h, int nb, int64_t rows, float* __restrict__ q) {
    const int64_t total = n_runs * nb, plane = rows * h;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = t / nb;
        const int b = (int)(t - k * nb);
        const float* vp = v + b * plane + (int64_t)run_id[k] * h;
        const float* sp = s + k * h;
        float acc = 0.f;
        for (int c = 0; c < h; ++c) acc = fmaf(vp[c], sp[c], acc);
        q[q_pos[k] * nb + b] = acc;
    }
}

// dcomp[r, b] (+)= sum of Q rows rel_ptr[r] .. rel_ptr[r+1]; thread t owns column t % nbc and every (T / nbc)-th row
constexpr int EC_RED_THREADS = 256;
__global__ __launch_bounds__(EC_RED_THREADS) void k_ec_basis_dcomp(const float* __restrict__ q, const int64_t* __restrict__ rel_ptr,
                                                                   int nb, int accumulate, float* __restrict__ dcomp) {
    __shared__ float part[EC_RED_THREADS];
    const int r = blockIdx.x, t = threadIdx.x;
    const int nbc = nb < EC_RED_THREADS ? nb : EC_RED_THREADS;
    const int per = EC_RED_THREADS / nbc;
    const int64_t j0 = rel_ptr[r], len = rel_ptr[r + 1] - j0;
    for (int bb = 0; bb < nb; bb += nbc) {
        const int b = bb + t % nbc;
        float acc = 0.f;
        if (t < per * nbc && b < nb)
            for (int64_t j = t / nbc; j < len; j += per) acc += q[(j0 + j) * nb + b];
        part[t] = acc;
        __syncthreads();
        if (t < nbc && b < nb) {
            float sum = 0.f;
            for (int i = 0; i < per; ++i) sum += part[i * nbc + t];
            float* o = dcomp + (int64_t)r * nb + b;
            *o = accumulate ? *o + sum : sum;
        }
        __syncthreads();
    }
}

// ---- head ----------------------------------------------------------------------------------------------------------------------
// one wave per row; lane c < C holds column c
__device__ __forceinline__ unsigned long long ec_ballot(bool p) { return __ballot(p); }

__global__ __launch_bounds__(256) void k_ec_head_fwd(const float* __restrict__ h, const int64_t* __restrict__ labels,
                                                     const int32_t* __restrict__ row_pos, int64_t n, int c_dim,
                                                     float* __restrict__ p, float* __restrict__ term, int32_t* __restrict__ correct) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool on = lane < c_dim;
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        const float x = on ? h[i * c_dim + lane] : -INFINITY;
        const float m = wave_max(x);
        const float e = on ? expf(x - m) : 0.f;
        const float pv = e / wave_sum(e);
        if (on) p[i * c_dim + lane] = pv;
        const int pos = row_pos ? row_pos[i] : -1;
        if (pos < 0) continue;
        // the reference's F.cross_entropy on the probabilities: logsumexp(p) - p[y]; argmax of p, ties to the lowest column
        const int y = (int)labels[i];
        const float pm = wave_max(on ? pv : -INFINITY);
        const float lse = pm + logf(wave_sum(on ? expf(pv - pm) : 0.f));
        const float py = wave_sum(lane == y ? pv : 0.f);
        const unsigned long long top = ec_ballot(on && pv == pm);
        const int first = top ? __ffsll((long long)top) - 1 : 0;
        if (lane == 0) {
            term[pos] = lse - py;
            correct[pos] = first == y ? 1 : 0;
        }
    }
}

// loss[s] = mean of term over set s (NaN for an empty set), count[s] = correct rows; sets are the slices off[s] .. off[s+1]
__global__ __launch_bounds__(256) void k_ec_head_finish(const float* __restrict__ term, const int32_t* __restrict__ correct,
                                                        const int64_t* __restrict__ off, float* __restrict__ loss,
                                                        int32_t* __restrict__ count) {
    __shared__ float ps[256];
    __shared__ int pc[256];
    const int t = threadIdx.x;
    for (int s = 0; s < 3; ++s) {
        const int64_t a = off[s], b = off[s + 1];
        float acc = 0.f;
        int cnt = 0;
        for (int64_t j = a + t; j < b; j += 256) {
            acc += term[j];
            cnt += correct[j];
        }
        ps[t] = acc;
        pc[t] = cnt;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w) {
                ps[t] += ps[t + w];
                pc[t] += pc[t + w];
            }
            __syncthreads();
        }
        if (t == 0) {
            loss[s] = b > a ? ps[0] / (float)(b - a) : __int_as_float(0x7fc00000);
            count[s] = pc[0];
        }
        __syncthreads();
    }
}

// dh = p * (dp - <dp, p>),  dp = grad_p (or 0) + [row in slice s] * gloss[s] / |slice s| * (softmax(p) - onehot(y))
__global__ __launch_bounds__(256) void k_ec_head_bwd(const float* __restrict__ p, const int64_t* __restrict__ labels,
                                                     const int32_t* __restrict__ row_pos, const int64_t* __restrict__ off,
                                                     const float* __restrict__ gloss, const float* __restrict__ grad_p, int64_t n,
                                                     int c_dim, float* __restrict__ dh) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool on = lane < c_dim;
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        const int pos = (row_pos && gloss) ? row_pos[i] : -1;
        if (pos < 0 && !grad_p) {
            if (on) dh[i * c_dim + lane] = 0.f;
            continue;
        }
        const float pv = on ? p[i * c_dim + lane] : 0.f;
        float dp = (grad_p && on) ? grad_p[i * c_dim + lane] : 0.f;
        if (pos >= 0) {
            const int s = pos < off[1] ? 0 : (pos < off[2] ? 1 : 2);
            const int y = (int)labels[i];
            const float pm = wave_max(on ? pv : -INFINITY);
            const float e = on ? expf(pv - pm) : 0.f;
            const float q = e / wave_sum(e);
            dp += gloss[s] / (float)(off[s + 1] - off[s]) * (q - (lane == y ? 1.f : 0.f));
        }
        if (!on) dp = 0.f;
        const float dot = wave_sum(pv * dp);
        if (on) dh[i * c_dim + lane] = pv * (dp - dot);
    }
}

}  // namespace gv

using namespace gv;

extern "C" int gv_ec_basis_rows_fwd(const float* v, const float* comp, const int32_t* run_id, const int32_t* run_rel, int64_t n_runs,
                                    int h, int nb, int num_rels, int64_t rows, float* msg, void* stream) {
    GV_REQUIRE(n_runs >= 0 && h > 0 && nb > 0 && num_rels > 0 && rows > 0, GV_ERR_SHAPE,
               "gv_ec_basis_rows_fwd: n_runs=%lld h=%d nb=%d num_rels=%d rows=%lld", (long long)n_runs, h, nb, num_rels,
               (long long)rows);
    if (n_runs == 0) return GV_OK;
    GV_REQUIRE(v && comp && run_id && run_rel && msg, GV_ERR_NULL, "gv_ec_basis_rows_fwd: NULL pointer");
    const int comp_bytes = num_rels * nb * (int)sizeof(float);
    const int grid = ec_grid(n_runs * h, 256);
    if ((int64_t)num_rels * nb * 4 <= EC_COMP_LDS_MAX) {
        static unsigned long long raised = 0;
        if (comp_bytes > 48 * 1024 && !raise_dynamic_lds((const void*)k_ec_basis_rows_fwd<true>, EC_COMP_LDS_MAX, raised,
                                                         "gv_ec_basis_rows_fwd"))
            return GV_ERR_SHAPE;
        hipLaunchKernelGGL(k_ec_basis_rows_fwd<true>, dim3(grid), dim3(256), comp_bytes, GV_ST, v, comp, run_id, run_rel, n_runs,
                           h, nb, num_rels, rows, msg);
    } else {
        hipLaunchKernelGGL(k_ec_basis_rows_fwd<false>, dim3(grid), dim3(256), 0, GV_ST, v, comp, run_id, run_rel, n_runs, h, nb,
                           num_rels, rows, msg);
    }
    return launch_status("gv_ec_basis_rows_fwd");
}

extern "C" int gv_ec_basis_rows_bwd(const float* v, const float* comp, const float* s, const int32_t* run_id, const int32_t* run_rel,
                                    const int64_t* run_ptr, int64_t n_groups, const int64_t* q_pos, const int64_t* rel_ptr,
                                    int64_t n_runs, int h, int nb, int num_rels, int64_t rows, float* dv, float* q, float* dcomp,
                                    int accumulate, void* stream) {
    GV_REQUIRE(n_runs >= 0 && n_groups >= 0 && n_groups <= n_runs && h > 0 && nb > 0 && num_rels > 0 && rows > 0, GV_ERR_SHAPE,
               "gv_ec_basis_rows_bwd: n_runs=%lld n_groups=%lld h=%d nb=%d num_rels=%d", (long long)n_runs,
               (long long)n_groups, h, nb, num_rels);
    GV_REQUIRE(dv || dcomp, GV_ERR_NULL, "gv_ec_basis_rows_bwd: neither dv nor dcomp");
    GV_REQUIRE(!dcomp || (q && q_pos && rel_ptr && v), GV_ERR_NULL, "gv_ec_basis_rows_bwd: dcomp needs q, q_pos, rel_ptr and v");
    if (n_runs > 0) {
        GV_REQUIRE(s && run_id && comp && run_rel && run_ptr, GV_ERR_NULL, "gv_ec_basis_rows_bwd: NULL pointer");
        if (dv)
            hipLaunchKernelGGL(k_ec_basis_dv, dim3(ec_grid(n_groups * nb * h, 256)), dim3(256), 0, GV_ST, s, comp, run_id, run_rel,
                               run_ptr, n_groups, h, nb, rows, accumulate, dv);
        if (dcomp)
            hipLaunchKernelGGL(k_ec_basis_q, dim3(ec_grid(n_runs * nb, 256)), dim3(256), 0, GV_ST, v, s, run_id, q_pos, n_runs, h,
                               nb, rows, q);
    }
    if (dcomp)
        hipLaunchKernelGGL(k_ec_basis_dcomp, dim3(num_rels), dim3(EC_RED_THREADS), 0, GV_ST, q, rel_ptr, nb, accumulate, dcomp);
    return launch_status("gv_ec_basis_rows_bwd");
}

extern "C" int gv_ec_head_fwd(const float* h, const int64_t* labels, const int32_t* row_pos, const int64_t* set_off, int64_t n,
                              int c, float* p, float* term, int32_t* correct, float* loss, int32_t* count, void* stream) {
    GV_REQUIRE(n >= 0 && c >= 1 && c <= GV_EC_HEAD_MAX_CLASSES, GV_ERR_SHAPE, "gv_ec_head_fwd: n=%lld c=%d (1 <= c <= %d)",
               (long long)n, c, GV_EC_HEAD_MAX_CLASSES);
    GV_REQUIRE(n == 0 || (h && p), GV_ERR_NULL, "gv_ec_head_fwd: NULL pointer");
    GV_REQUIRE(!row_pos || (labels && set_off && term && correct && loss && count), GV_ERR_NULL,
               "gv_ec_head_fwd: index sets need labels, set_off, term, correct, loss and count");
    if (n > 0)
        hipLaunchKernelGGL(k_ec_head_fwd, dim3(ec_grid(n, 4)), dim3(256), 0, GV_ST, h, labels, row_pos, n, c, p, term, correct);
    if (row_pos) hipLaunchKernelGGL(k_ec_head_finish, dim3(1), dim3(256), 0, GV_ST, term, correct, set_off, loss, count);
    return launch_status("gv_ec_head_fwd");
}

extern "C" int gv_ec_head_bwd(const float* p, const int64_t* labels, const int32_t* row_pos, const int64_t* set_off,
                              const float* gloss, const float* grad_p, int64_t n, int c, float* dh, void* stream) {
    GV_REQUIRE(n >= 0 && c >= 1 && c <= GV_EC_HEAD_MAX_CLASSES, GV_ERR_SHAPE, "gv_ec_head_bwd: n=%lld c=%d (1 <= c <= %d)",
               (long long)n, c, GV_EC_HEAD_MAX_CLASSES);
    if (n == 0) return GV_OK;
    GV_REQUIRE(p && dh, GV_ERR_NULL, "gv_ec_head_bwd: NULL pointer");
    GV_REQUIRE(!gloss || (row_pos && labels && set_off), GV_ERR_NULL, "gv_ec_head_bwd: the loss gradient needs row_pos, labels and set_off");
    hipLaunchKernelGGL(k_ec_head_bwd, dim3(ec_grid(n, 4)), dim3(256), 0, GV_ST, p, labels, row_pos, set_off, gloss, grad_p, n, c, dh);
    return launch_status("gv_ec_head_bwd");
}
