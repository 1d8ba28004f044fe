// TransE (Bordes et al. 2013; the OpenKE formulation of baselines/transe): negative sampling, the fused training step, the
// ordered sparse SGD update and the filtered L1 / L2 ranker.  No float atomics anywhere: every sum has a fixed order, so a step
// is bit-identical run to run and eager vs captured.  Row widths up to GV_TRANSE_MAX_DIM; a row is held by one wave, TE_C columns a lane.
//
// Sampler.  Positive b of a batch of B draws Philox(seed, tick) counter (b, stream, tick): word x picks the training triple
// (multiply-shift onto [0, n_train)), word y the Bernoulli coin (head corrupted iff (y >> 8) * 2^-24 < p_head[r]).  Negative j of
// positive b draws counter (b, stream + 0x10000 * (j + 1), tick), word x.  With a filter of k known answers out of V the word is
// mapped onto [0, V - k) and then to the u-th entity NOT in the sorted known list (binary search on list[j] - j); k == V or no
// filter: onto [0, V).  Layout (OpenKE): the B positives, then neg_ent blocks of B negatives.
//
// Step.  One wave per positive.  Every row is scored in OpenKE's 'normal' mode, ||(h + r) - t||_p, with h, r, t each passed through
// F.normalize (x / max(||x||_2, 1e-12)) when norm_flag is set.  The positive's rows are gathered and normalised once; a negative
// re-gathers only its corrupted side (the side whose id differs from the positive's; the tail when neither does).  Gradients of the
// uncorrupted sides are accumulated in registers over the negatives in j order, then the positive; one gradient row is written per
// occurrence: [h of b | t of b | corrupted side of (j, b)] for entities, [r of b] for relations.
//
// Ranker.  Distance of query q to entity j: ||q - n(E_j)||_p, summed over the columns in order with one accumulator
// (p = 2: fmaf(d, d, acc), then sqrtf).  The fused ranker, gv_transe_topk and gv_transe_distances share te_tile(), so their
// distances are the same bits.
//
// Top-k (gv_transe_topk).  te_tile()'s distances with the selection of gv_topk_scores (k_topk.h) on the key of -distance: smaller
// distance first, ties by lower id, NaN last; the distance matrix is never stored.
//
// Per-entity completion (gv_transe_entity_topk).  The same tile and selection with the relations walked inside a query entity's list:
// the query row en[a] +- rn[r] is formed while it is staged (te_tile_with), the candidate id is r * N + x.
#include "common.h"
#include "k_query_args.h"
#include "k_topk.h"
#include "k_transe.h"

namespace gv {

#define GV_ST ((hipStream_t)stream)

constexpr int TE_C = GV_TRANSE_MAX_DIM / WAVE;     // columns per lane
constexpr float TE_EPS = 1e-12f;                    // F.normalize's eps

__device__ __forceinline__ void te_load(const float* __restrict__ row, int dim, int lane, float (&x)[TE_C]) {
#pragma unroll
    for (int c = 0; c < TE_C; ++c) {
        const int k = lane + c * WAVE;
        x[c] = k < dim ? row[k] : 0.f;
    }
}

// y = x / max(||x||_2, eps); returns ||x||_2 (the sum of squares in a fixed order)
__device__ __forceinline__ float te_normalize(const float (&x)[TE_C], float (&y)[TE_C], bool on) {
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < TE_C; ++c) ss = fmaf(x[c], x[c], ss);
    const float n = sqrtf(wave_sum(ss));
    const float den = fmaxf(n, TE_EPS);
#pragma unroll
    for (int c = 0; c < TE_C; ++c) y[c] = on ? x[c] / den : x[c];
    return n;
}

// F.normalize backward: gx = (gy - y <y, gy>) / ||x|| where ||x|| >= eps, gy / eps below it
__device__ __forceinline__ void te_normalize_bwd(const float (&y)[TE_C], float n, const float (&gy)[TE_C], float (&gx)[TE_C], bool on) {
    if (!on) {
#pragma unroll
        for (int c = 0; c < TE_C; ++c) gx[c] = gy[c];
        return;
    }
    if (n >= TE_EPS) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < TE_C; ++c) d = fmaf(y[c], gy[c], d);
        d = wave_sum(d);
#pragma unroll
        for (int c = 0; c < TE_C; ++c) gx[c] = (gy[c] - y[c] * d) / n;
    } else {
#pragma unroll
        for (int c = 0; c < TE_C; ++c) gx[c] = gy[c] / TE_EPS;
    }
}

// ||z||_p of z = (a + b) - c, and z itself
__device__ __forceinline__ float te_dist(const float (&a)[TE_C], const float (&b)[TE_C], const float (&c)[TE_C], float (&z)[TE_C],
                                         int p) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < TE_C; ++i) {
        z[i] = (a[i] + b[i]) - c[i];
        s = p == 1 ? s + fabsf(z[i]) : fmaf(z[i], z[i], s);
    }
    s = wave_sum(s);
    return p == 1 ? s : sqrtf(s);
}

// dz = g * d||z||_p / dz: sign(z) for p = 1, z / ||z|| for p = 2; 0 at z = 0 (torch's norm backward)
__device__ __forceinline__ void te_dist_bwd(const float (&z)[TE_C], float dist, float g, int p, float (&dz)[TE_C]) {
#pragma unroll
    for (int i = 0; i < TE_C; ++i) {
        if (p == 1) dz[i] = z[i] > 0.f ? g : (z[i] < 0.f ? -g : 0.f);
        else dz[i] = dist == 0.f ? 0.f : z[i] * (g / dist);
    }
}

__device__ __forceinline__ void te_store(float* __restrict__ row, int dim, int lane, const float (&x)[TE_C]) {
#pragma unroll
    for (int c = 0; c < TE_C; ++c) {
        const int k = lane + c * WAVE;
        if (k < dim) row[k] = x[c];
    }
}

// ---- sampler -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_transe_sample(const uint64_t* __restrict__ rng_state, uint32_t stream,
                                                       const int32_t* __restrict__ train, int64_t n_train, int n_ent,
                                                       const float* __restrict__ p_head, const int32_t* __restrict__ f_lo,
                                                       const int32_t* __restrict__ f_hi, const int32_t* __restrict__ f_ent_o,
                                                       const int32_t* __restrict__ f_ent_s, int B, int neg_ent,
                                                       int32_t* __restrict__ bh, int32_t* __restrict__ br, int32_t* __restrict__ bt,
                                                       uint32_t* __restrict__ draws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint64_t seed = rng_state[0], tick = rng_state[1];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), t0 = (uint32_t)tick, t1 = (uint32_t)(tick >> 32);
    const uint4 x = philox4x32_10(k0, k1, (uint32_t)b, stream, t0, t1);
    const int64_t i = (int64_t)(((uint64_t)x.x * (uint64_t)n_train) >> 32);
    const int h = train[3 * i], r = train[3 * i + 1], t = train[3 * i + 2];
    const bool head = p_head ? (float)(x.y >> 8) * (1.f / 16777216.f) < p_head[r] : false;
    bh[b] = h; br[b] = r; bt[b] = t;
    if (draws) { draws[(int64_t)b * (neg_ent + 2)] = x.x; draws[(int64_t)b * (neg_ent + 2) + 1] = x.y; }
    // the known answers of the corrupted side: heads of (?, r, t) when the head is replaced, tails of (h, r, ?) otherwise
    int lo = 0, k = 0;
    const int32_t* list = nullptr;
    if (f_lo) {
        const int64_t slot = 2 * i + (head ? 1 : 0);
        lo = f_lo[slot];
        k = f_hi[slot] - lo;
        list = (head ? f_ent_s : f_ent_o) + lo;
    }
    const bool filt = list && k < n_ent;
    const uint32_t range = filt ? (uint32_t)(n_ent - k) : (uint32_t)n_ent;
    for (int j = 0; j < neg_ent; ++j) {
        const uint32_t w = philox4x32_10(k0, k1, (uint32_t)b, stream + 0x10000u * (uint32_t)(j + 1), t0, t1).x;
        if (draws) draws[(int64_t)b * (neg_ent + 2) + 2 + j] = w;
        int u = (int)(((uint64_t)w * range) >> 32);
        if (filt) {              // the u-th entity not in list[0, k): u + #{list[m] - m <= u}
            int a = 0, z = k;
            while (a < z) {
                const int m = (a + z) >> 1;
                if (list[m] - m <= u) a = m + 1;
                else z = m;
            }
            u += a;
        }
        const int64_t o = (int64_t)B * (j + 1) + b;
        bh[o] = head ? u : h;
        br[o] = r;
        bt[o] = head ? t : u;
    }
}

// ---- fused step ----------------------------------------------------------------------------------
struct TeStepArgs {
    const float* ent;
    const float* rel;
    const int32_t* bh;
    const int32_t* br;
    const int32_t* bt;
    int B, neg_ent, dim, p, norm;
    float margin, adv_t, regul;
    float* g_ent;       // (2B + neg_ent * B, dim)
    float* g_rel;       // (B, dim)
    float* loss_part;   // (B)
    float* score;       // (B * (1 + neg_ent)) or NULL
    int32_t* occ_ent;   // ((2 + neg_ent) B) entity id of each gradient row of g_ent, or NULL
};

__global__ __launch_bounds__(256) void k_transe_step(TeStepArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int B = a.B, K = a.neg_ent, dim = a.dim, p = a.p;
    const bool on = a.norm != 0, adv = a.adv_t > 0.f;
    const int64_t N = (int64_t)B * (1 + K);
    const int ph = a.bh[b], pr = a.br[b], pt = a.bt[b];
    float xh[TE_C], xr[TE_C], xt[TE_C], yh[TE_C], yr[TE_C], yt[TE_C], z[TE_C];
    te_load(a.ent + (int64_t)ph * dim, dim, lane, xh);
    te_load(a.rel + (int64_t)pr * dim, dim, lane, xr);
    te_load(a.ent + (int64_t)pt * dim, dim, lane, xt);
    const float nh = te_normalize(xh, yh, on), nr = te_normalize(xr, yr, on), nt = te_normalize(xt, yt, on);
    const float ps = te_dist(yh, yr, yt, z, p);
    if (a.score && lane == 0) a.score[b] = ps;
    if (a.occ_ent && lane == 0) { a.occ_ent[b] = ph; a.occ_ent[B + b] = pt; }
    const float inv_bk = 1.f / (float)((int64_t)B * K);
    // adversarial weights: softmax(-n * T) over the positive's negatives (first pass: the scores, their max and sum)
    float wmax = -INFINITY, wsum = 0.f;
    if (adv) {
        for (int j = 0; j < K; ++j) {
            const int64_t o = (int64_t)B * (j + 1) + b;
            const int nhid = a.bh[o];
            const bool head = nhid != ph;
            float xc[TE_C], yc[TE_C];
            te_load(a.ent + (int64_t)(head ? nhid : a.bt[o]) * dim, dim, lane, xc);
            te_normalize(xc, yc, on);
            const float ns = head ? te_dist(yc, yr, yt, z, p) : te_dist(yh, yr, yc, z, p);
            const float v = -ns * a.adv_t;
            const float m2 = fmaxf(wmax, v);
            wsum = wsum * expf(wmax - m2) + expf(v - m2);
            wmax = m2;
        }
    }
    float gh[TE_C], gr[TE_C], gt[TE_C];
#pragma unroll
    for (int c = 0; c < TE_C; ++c) gh[c] = gr[c] = gt[c] = 0.f;
    float gp = 0.f, loss = 0.f;
    int n_head = 0;
    for (int j = 0; j < K; ++j) {
        const int64_t o = (int64_t)B * (j + 1) + b;
        const int nhid = a.bh[o];
        const bool head = nhid != ph;
        const int cid = head ? nhid : a.bt[o];
        n_head += head;
        float xc[TE_C], yc[TE_C], dz[TE_C], gyc[TE_C], gxc[TE_C];
        te_load(a.ent + (int64_t)cid * dim, dim, lane, xc);
        const float nc = te_normalize(xc, yc, on);
        const float ns = head ? te_dist(yc, yr, yt, z, p) : te_dist(yh, yr, yc, z, p);
        if (a.score && lane == 0) a.score[o] = ns;
        if (a.occ_ent && lane == 0) a.occ_ent[(int64_t)2 * B + (int64_t)j * B + b] = cid;
        const float w = adv ? expf(-ns * a.adv_t - wmax) / wsum : inv_bk;
        const float d = ps - ns, hinge = fmaxf(d, -a.margin);
        loss += adv ? w * hinge : hinge;
        // torch.max(x, -margin): the whole gradient to x above the margin, half of it at a tie
        const float gd = (d > -a.margin ? 1.f : (d == -a.margin ? 0.5f : 0.f)) * (adv ? w / (float)B : inv_bk);
        gp += gd;
        te_dist_bwd(z, ns, -gd, p, dz);
#pragma unroll
        for (int c = 0; c < TE_C; ++c) {
            gr[c] += dz[c];
            if (head) { gyc[c] = dz[c]; gt[c] -= dz[c]; }
            else { gh[c] += dz[c]; gyc[c] = -dz[c]; }
        }
        te_normalize_bwd(yc, nc, gyc, gxc, on);
        if (a.regul != 0.f) {
            const float cr = a.regul * 2.f / (3.f * (float)N * (float)dim);
#pragma unroll
            for (int c = 0; c < TE_C; ++c) gxc[c] = fmaf(cr, xc[c], gxc[c]);
        }
        te_store(a.g_ent + ((int64_t)2 * B + (int64_t)j * B + b) * dim, dim, lane, gxc);
    }
    {   // the positive, last (z held the negatives' differences: the positive's is formed again, the same bits)
        float zp[TE_C], dz[TE_C];
        te_dist(yh, yr, yt, zp, p);
        te_dist_bwd(zp, ps, gp, p, dz);
#pragma unroll
        for (int c = 0; c < TE_C; ++c) { gh[c] += dz[c]; gr[c] += dz[c]; gt[c] -= dz[c]; }
    }
    float gx[TE_C];
    const float cr = a.regul != 0.f ? a.regul * 2.f / (3.f * (float)N * (float)dim) : 0.f;
    te_normalize_bwd(yh, nh, gh, gx, on);
    if (cr != 0.f) {
#pragma unroll
        for (int c = 0; c < TE_C; ++c) gx[c] = fmaf(cr * (float)(1 + K - n_head), xh[c], gx[c]);
    }
    te_store(a.g_ent + (int64_t)b * dim, dim, lane, gx);
    te_normalize_bwd(yt, nt, gt, gx, on);
    if (cr != 0.f) {
#pragma unroll
        for (int c = 0; c < TE_C; ++c) gx[c] = fmaf(cr * (float)(1 + n_head), xt[c], gx[c]);
    }
    te_store(a.g_ent + ((int64_t)B + b) * dim, dim, lane, gx);
    te_normalize_bwd(yr, nr, gr, gx, on);
    if (cr != 0.f) {
#pragma unroll
        for (int c = 0; c < TE_C; ++c) gx[c] = fmaf(cr * (float)(1 + K), xr[c], gx[c]);
    }
    te_store(a.g_rel + (int64_t)b * dim, dim, lane, gx);
    if (a.regul != 0.f) {   // this positive's share of regul_rate * (mean h^2 + mean t^2 + mean r^2) / 3 over the N rows
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < TE_C; ++c)
            s += (float)(1 + K - n_head) * (xh[c] * xh[c]) + (float)(1 + n_head) * (xt[c] * xt[c]) + (float)(1 + K) * (xr[c] * xr[c]);
        for (int j = 0; j < K; ++j) {
            const int64_t o = (int64_t)B * (j + 1) + b;
            const int nhid = a.bh[o];
            float xc[TE_C];
            te_load(a.ent + (int64_t)(nhid != ph ? nhid : a.bt[o]) * dim, dim, lane, xc);
#pragma unroll
            for (int c = 0; c < TE_C; ++c) s = fmaf(xc[c], xc[c], s);
        }
        loss = loss * (adv ? 1.f / (float)B : inv_bk) + a.regul * wave_sum(s) / (3.f * (float)N * (float)dim);
    } else {
        loss = loss * (adv ? 1.f / (float)B : inv_bk);
    }
    if (lane == 0) a.loss_part[b] = loss;
}

// ---- ordered reduction + SGD -----------------------------------------------------------------------
// One wave per table row: the row's occurrences (perm[rowptr[s] .. rowptr[s+1])) summed in occurrence order, then p += -lr * g.
// Rows without occurrences are not written.  The last block sums the loss partials (fixed order) into loss_out[0] and adds that
// to the double epoch accumulator.
__global__ __launch_bounds__(256) void k_transe_apply(float* __restrict__ ent, int n_ent, const float* __restrict__ g_ent,
                                                      const int32_t* __restrict__ perm_e, const int32_t* __restrict__ rowptr_e,
                                                      float* __restrict__ rel, int n_rel, const float* __restrict__ g_rel,
                                                      const int32_t* __restrict__ perm_r, const int32_t* __restrict__ rowptr_r,
                                                      int dim, float lr, const float* __restrict__ loss_part, int B, float margin,
                                                      float* __restrict__ loss_out, double* __restrict__ epoch_acc, int row_blocks) {
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x == row_blocks) {
        if (threadIdx.x >= 64) return;
        float s = 0.f;
        for (int i = lane; i < B; i += 64) s += loss_part[i];
        s = wave_sum(s) + margin;
        if (lane == 0) {
            loss_out[0] = s;
            if (epoch_acc) epoch_acc[0] += (double)s;
        }
        return;
    }
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    float* table;
    const float* g;
    const int32_t *perm, *rowptr;
    int s;
    if (w < n_ent) { table = ent; g = g_ent; perm = perm_e; rowptr = rowptr_e; s = w; }
    else if (w < n_ent + n_rel) { table = rel; g = g_rel; perm = perm_r; rowptr = rowptr_r; s = w - n_ent; }
    else return;
    const int lo = rowptr[s], hi = rowptr[s + 1];
    if (lo == hi) return;
    for (int k = lane; k < dim; k += 64) {
        float acc = 0.f;
        for (int i = lo; i < hi; ++i) acc += g[(int64_t)perm[i] * dim + k];
        float* q = table + (int64_t)s * dim + k;
        *q = *q + (-lr) * acc;
    }
}

// ---- ordered reduction + torch.optim rule ----------------------------------------------------------
// k_transe_apply's work split, order of summation and loss block; the rule applied to the row's summed g is torch.optim's SGD,
// Adagrad, Adadelta or Adam at torch's defaults, with the coupled L2 decay g += wd * p first.  Dense semantics: under Adadelta,
// Adam or any wd != 0 every row of both tables is updated (an untouched row has g = 0: its moments still move it, its averages
// decay, it shrinks); under SGD / Adagrad at wd == 0 an untouched row is the identity and is not written.  The step number t
// (1-based, int64 on the device) is only read: something ahead of this launch advances it.  The scalars that depend on t are
// formed in double from the double hyper-parameters, as torch forms them in Python floats, and rounded to float once.
struct TeOptArgs {
    float* ent;
    float* rel;
    float* s1_ent;              // Adagrad: sum; Adadelta: square_avg; Adam: exp_avg
    float* s2_ent;              // Adadelta: acc_delta; Adam: exp_avg_sq
    float* s1_rel;
    float* s2_rel;
    const float* g_ent;
    const float* g_rel;
    const int32_t* perm_e;
    const int32_t* rowptr_e;
    const int32_t* perm_r;
    const int32_t* rowptr_r;
    const int64_t* step_t;
    const float* loss_part;
    float* loss_out;
    double* epoch_acc;
    double lr, wd, lr_decay;
    int n_ent, n_rel, dim, method, B, row_blocks;
    float margin;
};

constexpr double TE_ADADELTA_RHO = 0.9, TE_ADADELTA_EPS = 1e-6, TE_ADAGRAD_EPS = 1e-10;
constexpr double TE_ADAM_B1 = 0.9, TE_ADAM_B2 = 0.999, TE_ADAM_EPS = 1e-8;

__global__ __launch_bounds__(256) void k_transe_apply_opt(const TeOptArgs a) {
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x == a.row_blocks) {
        if (threadIdx.x >= 64) return;
        float s = 0.f;
        for (int i = lane; i < a.B; i += 64) s += a.loss_part[i];
        s = wave_sum(s) + a.margin;
        if (lane == 0) {
            a.loss_out[0] = s;
            if (a.epoch_acc) a.epoch_acc[0] += (double)s;
        }
        return;
    }
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    float *table, *s1, *s2;
    const float* g;
    const int32_t *perm, *rowptr;
    int s;
    if (w < a.n_ent) { table = a.ent; s1 = a.s1_ent; s2 = a.s2_ent; g = a.g_ent; perm = a.perm_e; rowptr = a.rowptr_e; s = w; }
    else if (w < a.n_ent + a.n_rel) {
        table = a.rel; s1 = a.s1_rel; s2 = a.s2_rel; g = a.g_rel; perm = a.perm_r; rowptr = a.rowptr_r; s = w - a.n_ent;
    } else return;
    const int method = a.method, dim = a.dim;
    const bool decay = a.wd != 0.0;
    const int lo = rowptr[s], hi = rowptr[s + 1];
    if (lo == hi && !decay && (method == GV_TRANSE_OPT_SGD || method == GV_TRANSE_OPT_ADAGRAD)) return;
    const float wd = (float)a.wd, lr = (float)a.lr;
    // per-step scalars (wave-uniform): Adagrad's clr; Adam's lr / bc1 and sqrt(bc2)
    float c0 = 0.f, c1 = 0.f;
    if (method == GV_TRANSE_OPT_ADAGRAD) {
        c0 = (float)(a.lr / (1.0 + (double)(a.step_t[0] - 1) * a.lr_decay));
    } else if (method == GV_TRANSE_OPT_ADAM) {
        const double t = (double)a.step_t[0];
        c0 = (float)(a.lr / (1.0 - pow(TE_ADAM_B1, t)));
        c1 = (float)sqrt(1.0 - pow(TE_ADAM_B2, t));
    }
    // every column's sum runs over the occurrences in perm order from 0, as k_transe_apply's does (the same bits); the row's
    // columns are summed side by side and four occurrences are fetched at a time, so a long run waits for a quarter of its
    // occurrences' two dependent loads (perm, then the gradient row) instead of for each one once per 64 columns
    float acc[TE_C];
#pragma unroll
    for (int c = 0; c < TE_C; ++c) acc[c] = 0.f;
    int i = lo;
    for (; i + 4 <= hi; i += 4) {
        const int32_t o0 = perm[i], o1 = perm[i + 1], o2 = perm[i + 2], o3 = perm[i + 3];
        float x0[TE_C], x1[TE_C], x2[TE_C], x3[TE_C];
        te_load(g + (int64_t)o0 * dim, dim, lane, x0);
        te_load(g + (int64_t)o1 * dim, dim, lane, x1);
        te_load(g + (int64_t)o2 * dim, dim, lane, x2);
        te_load(g + (int64_t)o3 * dim, dim, lane, x3);
#pragma unroll
        for (int c = 0; c < TE_C; ++c) acc[c] = (((acc[c] + x0[c]) + x1[c]) + x2[c]) + x3[c];
    }
    for (; i < hi; ++i) {
        float x0[TE_C];
        te_load(g + (int64_t)perm[i] * dim, dim, lane, x0);
#pragma unroll
        for (int c = 0; c < TE_C; ++c) acc[c] += x0[c];
    }
    const int64_t base = (int64_t)s * dim;
#pragma unroll
    for (int c = 0; c < TE_C; ++c) {
        const int k = lane + c * WAVE;
        if (k >= dim) continue;
        float* q = table + base + k;
        const float p = *q;
        float gk = acc[c];
        if (decay) gk = gk + wd * p;
        if (method == GV_TRANSE_OPT_SGD) {
            *q = p + (-lr) * gk;
        } else if (method == GV_TRANSE_OPT_ADAGRAD) {
            const float sum = s1[base + k] + gk * gk;
            s1[base + k] = sum;
            *q = p - c0 * gk / (sqrtf(sum) + (float)TE_ADAGRAD_EPS);
        } else if (method == GV_TRANSE_OPT_ADADELTA) {
            const float rho = (float)TE_ADADELTA_RHO, one_rho = (float)(1.0 - TE_ADADELTA_RHO), eps = (float)TE_ADADELTA_EPS;
            const float sq = rho * s1[base + k] + one_rho * (gk * gk);
            const float ad = s2[base + k];
            const float d = sqrtf(ad + eps) / sqrtf(sq + eps) * gk;
            s1[base + k] = sq;
            s2[base + k] = rho * ad + one_rho * (d * d);
            *q = p - lr * d;
        } else {
            const float w1 = (float)(1.0 - TE_ADAM_B1), b2 = (float)TE_ADAM_B2, w2 = (float)(1.0 - TE_ADAM_B2);
            const float m0 = s1[base + k];
            const float m = m0 + w1 * (gk - m0);
            const float v = b2 * s2[base + k] + w2 * (gk * gk);
            s1[base + k] = m;
            s2[base + k] = v;
            *q = p - c0 * m / (sqrtf(v) / c1 + (float)TE_ADAM_EPS);
        }
    }
}

// ---- queries and table normalisation ---------------------------------------------------------------
// q[i] = n(ent[a[i]]) + n(rel[r[i]]) (tail queries) or n(ent[a[i]]) - n(rel[r[i]]) (head queries); with rel == NULL: q[i] = n(ent[i])
__global__ __launch_bounds__(256) void k_transe_queries(const float* __restrict__ ent, const float* __restrict__ rel,
                                                        const int32_t* __restrict__ ai, const int32_t* __restrict__ ri, int64_t m,
                                                        int dim, int head, int norm, float* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    float x[TE_C], y[TE_C];
    te_load(ent + (int64_t)(rel ? ai[i] : i) * dim, dim, lane, x);
    te_normalize(x, y, norm != 0);
    if (rel) {
        float xr[TE_C], yr[TE_C];
        te_load(rel + (int64_t)ri[i] * dim, dim, lane, xr);
        te_normalize(xr, yr, norm != 0);
#pragma unroll
        for (int c = 0; c < TE_C; ++c) y[c] = head ? y[c] - yr[c] : y[c] + yr[c];
    }
    te_store(q + i * dim, dim, lane, y);
}

// ---- distances and the fused ranker --------------------------------------------------------------------
constexpr int TE_KC = 32;   // columns per LDS stage of a TE_TQ x TE_TE tile (k_transe.h, with te_pair_term)

// acc[4][4] for the tile's query rows 4 ty .. and entities e0 + 4 tx ..: the columns in order, one accumulator per pair.
// q_at(row, c): column c of the tile's query row `row` as it is staged (0 past the last row or column) -- te_tile reads a stored
// query matrix, gv_transe_entity_topk forms the row on the way.
template <class QAt>
__device__ __forceinline__ void te_tile_with(QAt q_at, const float* __restrict__ en, int v, int dim, int p, int e0,
                                             float (*qs)[TE_TQ + 4], float (*es)[TE_TE + 4], float (&acc)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < dim; k0 += TE_KC) {
        __syncthreads();
        for (int x = tid; x < TE_TQ * TE_KC; x += 256) {
            const int row = x / TE_KC, k = x % TE_KC;
            qs[k][row] = q_at(row, k0 + k);
            const int ej = e0 + row;
            es[k][row] = (ej < v && k0 + k < dim) ? en[(int64_t)ej * dim + k0 + k] : 0.f;
        }
        __syncthreads();
        const int kn = min(TE_KC, dim - k0);
        for (int k = 0; k < kn; ++k) {
            const float4 qa = *reinterpret_cast<const float4*>(&qs[k][4 * ty]);
            const float4 eb = *reinterpret_cast<const float4*>(&es[k][4 * tx]);
            const float qv[4] = {qa.x, qa.y, qa.z, qa.w}, ev[4] = {eb.x, eb.y, eb.z, eb.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = te_pair_term(acc[a][b], qv[a], ev[b], p);
        }
    }
    if (p == 2) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = sqrtf(acc[a][b]);
    }
}

// te_tile_with with the tile's entity rows supplied by the caller as well: e_at(row, c) is column c of the tile's entity row `row` as
// it is staged (0 for a row that holds none, or past the last column) -- gv_transe_entity_topk_typed gathers the rows through member
// ids.  The same staging, the same column order, the same per-pair chain: a gathered row's distances are te_tile's bits.
template <class QAt, class EAt>
__device__ __forceinline__ void te_tile_gather(QAt q_at, EAt e_at, int dim, int p, float (*qs)[TE_TQ + 4], float (*es)[TE_TE + 4],
                                               float (&acc)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < dim; k0 += TE_KC) {
        __syncthreads();
        for (int x = tid; x < TE_TQ * TE_KC; x += 256) {
            const int row = x / TE_KC, k = x % TE_KC;
            qs[k][row] = q_at(row, k0 + k);
            es[k][row] = e_at(row, k0 + k);
        }
        __syncthreads();
        const int kn = min(TE_KC, dim - k0);
        for (int k = 0; k < kn; ++k) {
            const float4 qa = *reinterpret_cast<const float4*>(&qs[k][4 * ty]);
            const float4 eb = *reinterpret_cast<const float4*>(&es[k][4 * tx]);
            const float qv[4] = {qa.x, qa.y, qa.z, qa.w}, ev[4] = {eb.x, eb.y, eb.z, eb.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = te_pair_term(acc[a][b], qv[a], ev[b], p);
        }
    }
    if (p == 2) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = sqrtf(acc[a][b]);
    }
}

// the tile of rows q0 .. of a stored query matrix q (m, dim)
__device__ __forceinline__ void te_tile(const float* __restrict__ q, int64_t m, const float* __restrict__ en, int v, int dim, int p,
                                        int64_t q0, int e0, float (*qs)[TE_TQ + 4], float (*es)[TE_TE + 4], float (&acc)[4][4]) {
    te_tile_with(
        [&](int row, int c) {
            const int64_t qi = q0 + row;
            return (qi < m && c < dim) ? q[qi * dim + c] : 0.f;
        },
        en, v, dim, p, e0, qs, es, acc);
}

__global__ __launch_bounds__(256) void k_transe_distances(const float* __restrict__ q, int64_t m, const float* __restrict__ en, int v,
                                                          int dim, int p, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float qs[TE_KC][TE_TQ + 4];
    __shared__ __attribute__((aligned(16))) float es[TE_KC][TE_TE + 4];
    const int64_t q0 = (int64_t)blockIdx.x * TE_TQ;
    const int e0 = blockIdx.y * TE_TE;
    float acc[4][4];
    te_tile(q, m, en, v, dim, p, q0, e0, qs, es, acc);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t qi = q0 + 4 * ty + a;
            const int ej = e0 + 4 * tx + b;
            if (qi < m && ej < v) out[qi * v + ej] = acc[a][b];
        }
}

// counts[0][i] = 2 #better + #equal (raw), counts[1][i] the same over the entities not listed in f_ent[f_lo[i], f_hi[i]) -- the
// rule of ranking.sort_and_rank on score = -distance: j != target is better when !(d_j >= d_target) (NaN on either side), equal
// when d_j == d_target.  Block (x, y) takes query tile x and entity tiles y, y + gridDim.y, ...; integer atomics add the counts.
// CAND (gv_transe_rank_constrained): raw_c / filt_c are the same counts over the members of the query's candidate set only (TopkCand,
// k_topk.h).  The tile's two set words sit in LDS next to the filter word, loaded by the second wave while the first builds the
// filter word; without a filter (f_lo NULL) neither filtered count is written.
template <bool CAND>
__global__ __launch_bounds__(256) void k_transe_rank(const float* __restrict__ q, int64_t m, const float* __restrict__ en, int v,
                                                     int dim, int p, const int32_t* __restrict__ target,
                                                     const int32_t* __restrict__ f_lo, const int32_t* __restrict__ f_hi,
                                                     const int32_t* __restrict__ f_ent, int32_t* __restrict__ raw,
                                                     int32_t* __restrict__ filt, const TopkCand cs, int32_t* __restrict__ raw_c,
                                                     int32_t* __restrict__ filt_c) {
    __shared__ __attribute__((aligned(16))) float qs[TE_KC][TE_TQ + 4];
    __shared__ __attribute__((aligned(16))) float es[TE_KC][TE_TE + 4];
    __shared__ float dt_s[TE_TQ];
    __shared__ unsigned long long mask_s[CAND ? 2 * TE_TQ : TE_TQ];       // the tile's filter word per row (CAND: + the set's)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * TE_TQ;
    if (tid < TE_TQ) {     // the target's distance, with te_tile's per-pair arithmetic
        const int64_t qi = q0 + tid;
        float acc = 0.f;
        if (qi < m) {
            const float* qr = q + qi * dim;
            const float* er = en + (int64_t)target[qi] * dim;
            for (int k = 0; k < dim; ++k) acc = te_pair_term(acc, qr[k], er[k], p);
            if (p == 2) acc = sqrtf(acc);
        }
        dt_s[tid] = acc;
    }
    int cr[4] = {0, 0, 0, 0}, cf[4] = {0, 0, 0, 0}, crc[4] = {0, 0, 0, 0}, cfc[4] = {0, 0, 0, 0};
    const int n_tiles = (v + TE_TE - 1) / TE_TE;
    for (int et = blockIdx.y; et < n_tiles; et += gridDim.y) {
        const int e0 = et * TE_TE;
        __syncthreads();
        if (tid < TE_TQ) {
            unsigned long long mk = 0;
            const int64_t qi = q0 + tid;
            if (f_lo && qi < m) {
                int a = f_lo[qi], z = f_hi[qi];
                while (a < z) {           // first listed id >= e0
                    const int mid = (a + z) >> 1;
                    if (f_ent[mid] < e0) a = mid + 1;
                    else z = mid;
                }
                for (int x = a; x < f_hi[qi] && f_ent[x] < e0 + TE_TE; ++x) mk |= 1ull << (f_ent[x] - e0);
            }
            mask_s[tid] = mk;
        } else if (CAND && tid < 2 * TE_TQ) {
            mask_s[tid] = topk_cand_pair(cs, q0 + tid - TE_TQ, m, e0, v);
        }
        float acc[4][4];
        te_tile(q, m, en, v, dim, p, q0, e0, qs, es, acc);    // its first barrier publishes dt_s / mask_s
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int row = 4 * ty + a;
            const int64_t qi = q0 + row;
            if (qi >= m) continue;
            const float dt = dt_s[row];
            const unsigned long long mk = mask_s[row];
            const int tg = target[qi];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = 4 * tx + b, ej = e0 + col;
                if (ej >= v || ej == tg) continue;
                const float d = acc[a][b];
                const int c = !(d >= dt) ? 2 : (d == dt ? 1 : 0);
                cr[a] += c;
                if (!(mk >> col & 1ull)) cf[a] += c;
                if (CAND && (mask_s[TE_TQ + row] >> col & 1ull)) {
                    crc[a] += c;
                    if (!(mk >> col & 1ull)) cfc[a] += c;
                }
            }
        }
    }
    // the 16 lanes of a query row hold its partial counts: sum them, one atomic per query and kind
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        for (int off = 8; off >= 1; off >>= 1) {
            cr[a] += __shfl_xor(cr[a], off, 16);
            cf[a] += __shfl_xor(cf[a], off, 16);
            if (CAND) {
                crc[a] += __shfl_xor(crc[a], off, 16);
                cfc[a] += __shfl_xor(cfc[a], off, 16);
            }
        }
        const int64_t qi = q0 + 4 * ty + a;
        if (tx == 0 && qi < m) {
            atomicAdd(&raw[qi], cr[a]);
            if (!CAND || f_lo) atomicAdd(&filt[qi], cf[a]);
            if (CAND) {
                atomicAdd(&raw_c[qi], crc[a]);
                if (f_lo) atomicAdd(&filt_c[qi], cfc[a]);
            }
        }
    }
}


// ---- fused top-k: te_tile() + the selection epilogue of gv_topk_scores ------------------------------------------------------------
// Workgroup (x, y) owns query tile x and sweeps span y of 64-entity tiles in ascending id order.  The 16 distances a lane holds
// after te_tile() go through LDS (ds) into one lane per column: wave w takes rows 16 w .. 16 w + 15, keys the column's distance as
// topk_key(-d, id) -- larger key = smaller distance, ties by lower id, NaN below every number -- and inserts what beats the row's
// running k-th key into the row's sorted LDS list.  Columns past v and listed ids get key 0 (no candidate).  The span's lists go to
// the workspace; k_topk_merge merges them, one wave per row, and TopkOut<int64_t, te_key_dist> decodes.  Nothing depends on the span
// count: every span list is the exact best k of its columns under a strict total order, and so is the merge.  Set-up, row loop and
// hand-on are topk_span_clear / topk_span_select / topk_span_hand_on of k_topk.h; the lambdas below are what is this kernel's own.
struct TeTopkParams {
    const float* q;
    const float* en;
    const int32_t* filt_lo;       // NULL: no filter
    const int32_t* filt_hi;
    const int32_t* filt_ent;
    int64_t m;
    int v, dim, p;
    int n_ent;                    // length of filt_ent: every range is clamped into it
    int topk;                     // 1..TOPK_MAX
    int span_tiles, n_spans;
    unsigned long long* part;     // [m][n_spans][topk] keys, each span's list sorted descending
    TopkCand cs;                  // CAND only (gv_transe_topk_constrained): non-members get key 0 as well
};

constexpr int TE_LDD = TE_TE + 4;      // row stride of the distance tile: float4 stores stay 16-byte aligned

template <int NK, bool CAND>
__global__ __launch_bounds__(256) void k_transe_topk_span(const TeTopkParams tp) {
    __shared__ __attribute__((aligned(16))) float qs[TE_KC][TE_TQ + 4];
    __shared__ __attribute__((aligned(16))) float es[TE_KC][TE_TE + 4];
    __shared__ __attribute__((aligned(16))) float ds[TE_TQ * TE_LDD];     // the tile's distances, row-major
    __shared__ unsigned long long thr[TE_TQ];                             // each row's k-th key
    __shared__ int cur[TE_TQ], fhi[TE_TQ], nxt[TE_TQ];                    // filter cursor (k_topk.h)
    __shared__ int fl[4][64];
    extern __shared__ unsigned long long lists[];                         // [TE_TQ][topk]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, tx = tid & 15, ty = tid >> 4;
    const int k = tp.topk;
    const int64_t q0 = (int64_t)blockIdx.x * TE_TQ;
    const int t_begin = blockIdx.y * tp.span_tiles;
    const int t_end = min(t_begin + tp.span_tiles, (tp.v + TE_TE - 1) / TE_TE);
    const bool filtered = tp.filt_lo != nullptr;
    topk_span_clear<TE_TQ>(lists, k, fl, thr, lane, wid, [&](int rl) {
        topk_filter_begin(tp.filt_lo, tp.filt_hi, tp.filt_ent, tp.n_ent, filtered && q0 + rl < tp.m, q0 + rl, t_begin * TE_TE,
                          &cur[rl], &fhi[rl], &nxt[rl]);
    });
    const uint32_t* cand_row = CAND ? topk_cand_row(tp.cs, q0 + wid * (TE_TQ / 4), tp.m, lane) : nullptr;
    for (int t = t_begin; t < t_end; ++t) {
        const int e0 = t * TE_TE;
        const unsigned cand_w = CAND ? topk_cand_word(cand_row, e0, tp.v, lane) : 0u;      // lands under te_tile
        float acc[4][4];
        // te_tile's first barrier publishes the set-up above and ends the last tile's reads of ds
        te_tile(tp.q, tp.m, tp.en, tp.v, tp.dim, tp.p, q0, e0, qs, es, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a)
            *reinterpret_cast<float4*>(&ds[(4 * ty + a) * TE_LDD + 4 * tx]) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        __syncthreads();
        const int col = e0 + lane;
        topk_span_select<NK, TE_TQ>(q0, tp.m, lists, thr, k, lane, wid, [&](int rl, int i) {
            unsigned long long key = col < tp.v ? topk_key(-ds[rl * TE_LDD + lane], col) : 0ull;
            if (filtered && nxt[rl] < e0 + TE_TE &&
                topk_filter_window(tp.filt_ent, e0, (t - t_begin) * TE_TQ + rl + 1, lane, &cur[rl], &fhi[rl], &nxt[rl], fl[wid]))
                key = 0ull;
            if (CAND && !topk_cand_member(cand_w, i, lane)) key = 0ull;
            return key;
        });
    }
    topk_span_hand_on<TE_TQ>(q0, tp.m, lists, k, tp.part, tp.n_spans, lane, wid);
}

// the key of -distance back to the distance: key 0 (no candidate) -> +inf; zero -> +0; NaN -> the one quiet NaN
__device__ __forceinline__ float te_key_dist(unsigned long long key) {
    const float x = topk_key_logit(key);                 // -distance, never -0
    const unsigned b = __float_as_uint(x) ^ 0x80000000u;
    return x != x ? x : __uint_as_float(b == 0x80000000u ? 0u : b);
}

// ---- per-entity completion (gv_transe_entity_topk): one list per query entity over ALL relations ---------------------------------
// Query row i is entity a = ents[i]; its candidates are the pairs (r, x) at distance ||(en[a] +- rn[r]) - en[x]||_p -- k_transe_topk_span
// with the relations walked INSIDE the row's list, as k_entity_topk_span (k_gemm.hip) does for DistMult: neither an (entity x
// relation) query matrix nor m * R * k intermediate results exist.  The columns of a row are the sequence of (relation, 64-entity
// tile) pairs, r-major: tile t = r * col_tiles + ct, candidate id = r * N + x (< 2^31), so the ordered key says "distance, then
// relation, then entity".  A workgroup owns a 64-row tile of query entities and a contiguous span of that sequence.  The query row is
// made while te_tile_with stages it: en[a][c] + rn[r][c] (head: -), one f32 add each -- the value k_transe_queries stores -- so the
// distances are gv_transe_distances' bits.  At the first tile of a relation (and of the span) the 64 rows' filter cursors are
// re-opened on key a * R + r.
struct TeEntityTopkParams {
    const float* en;              // [n, dim]
    const float* rn;              // [num_rels, dim]
    const int32_t* ents;          // [m] query entities; an id outside [0, n) is a row without candidates
    const int32_t* filt_lo;       // key a * R + r; NULL: no filter
    const int32_t* filt_hi;
    const int32_t* filt_ent;
    int m, n, num_rels, dim, p, head, exclude_self;
    int n_ent;                    // length of filt_ent: every range is clamped into it
    int topk;                     // 1..TOPK_MAX
    int span_tiles, n_spans;      // (relation, entity tile) pairs per span (blockIdx.y = span)
    unsigned long long* part;     // [m][n_spans][topk]
};

template <int NK>
__global__ __launch_bounds__(256) void k_transe_entity_topk_span(const TeEntityTopkParams tp) {
    __shared__ __attribute__((aligned(16))) float qs[TE_KC][TE_TQ + 4];
    __shared__ __attribute__((aligned(16))) float es[TE_KC][TE_TE + 4];
    __shared__ __attribute__((aligned(16))) float ds[TE_TQ * TE_LDD];     // the tile's distances, row-major
    __shared__ unsigned long long thr[TE_TQ];                             // each row's k-th key
    __shared__ int cur[TE_TQ], fhi[TE_TQ], nxt[TE_TQ];                    // filter cursor (k_topk.h)
    __shared__ int fl[4][64];
    __shared__ int ent_s[TE_TQ];                                          // the rows' entities (-1: no such row)
    extern __shared__ unsigned long long lists[];                         // [TE_TQ][topk]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, tx = tid & 15, ty = tid >> 4;
    const int k = tp.topk, dim = tp.dim;
    const int m0 = blockIdx.x * TE_TQ;
    const int col_tiles = (tp.n + TE_TE - 1) / TE_TE;
    const int t_begin = blockIdx.y * tp.span_tiles;
    const int t_end = min(t_begin + tp.span_tiles, tp.num_rels * col_tiles);
    const bool filtered = tp.filt_lo != nullptr, head = tp.head != 0;
    // topk_span_clear's lines with the threshold cleared AFTER the entity's fetch: through the shared set-up (threshold first) the
    // kernel is one instruction shorter, its loops sit 4 bytes earlier and the fused route measured 1.7 - 3.2 % slower (NOTES.md)
    for (int i = tid; i < TE_TQ * k; i += 256) lists[i] = 0ull;
    fl[wid][lane] = 0;
    if (tid < TE_TQ) {
        topk_pair_entity(tp.ents, m0, tid, tp.m, tp.n, ent_s);
        thr[tid] = 0ull;
    }
    TopkPairWalk walk(t_begin, col_tiles);
    for (int t = t_begin; t < t_end; ++t) {
        const TopkPairTile tile = walk.step(col_tiles, t == t_begin);
        const int e0 = tile.c0;
        const float* __restrict__ rr = tp.rn + (size_t)tile.r * dim;
        float acc[4][4];
        // te_tile_with's first barrier publishes the set-up above and ends the last tile's reads of ds and of the cursors
        te_tile_with(
            [&](int row, int c) {
                const int a = ent_s[row];
                if (a < 0 || c >= dim) return 0.f;
                const float x = tp.en[(size_t)a * dim + c], y = rr[c];
                return head ? x - y : x + y;
            },
            tp.en, tp.n, dim, tp.p, e0, qs, es, acc);
        // (every wave is past te_tile_with's last barrier: nobody still reads the previous relation's cursors)
        if (tile.opens && tid < TE_TQ)
            topk_pair_reopen(tp.filt_lo, tp.filt_hi, tp.filt_ent, tp.n_ent, ent_s, tp.num_rels, tile, cur, fhi, nxt);
#pragma unroll
        for (int a = 0; a < 4; ++a)
            *reinterpret_cast<float4*>(&ds[(4 * ty + a) * TE_LDD + 4 * tx]) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        __syncthreads();
        const int col = e0 + lane;
        topk_span_select<NK, TE_TQ>(m0, tp.m, lists, thr, k, lane, wid, [&](int rl, int) {
            const int a = ent_s[rl];
            unsigned long long key = col < tp.n ? topk_key(-ds[rl * TE_LDD + lane], tile.r * tp.n + col) : 0ull;
            if (filtered && nxt[rl] < e0 + TE_TE &&
                topk_filter_window(tp.filt_ent, e0, (int)((unsigned)(t - t_begin) * TE_TQ + rl + 1u), lane, &cur[rl], &fhi[rl], &nxt[rl],
                                   fl[wid]))
                key = 0ull;
            return tp.exclude_self && col == a ? 0ull : key;
        }, [&](int rl) { return ent_s[rl] >= 0; });
    }
    topk_span_hand_on<TE_TQ>(m0, tp.m, lists, k, tp.part, tp.n_spans, lane, wid);
}

// ---- per-entity completion among TYPE-CORRECT facts (gv_transe_entity_topk_typed) -------------------------------------------------
// k_transe_entity_topk_span with a row's columns taken from the relations' candidate member lists (TopkTyped, k_topk.h), as
// k_entity_topk_typed_span (k_gemm.hip) does for DistMult: the r-major sequence of (relation, 64-member tile of set cand_base + r)
// pairs.  The tile's entity rows are gathered through its 64 ids (te_tile_gather: the same columns in the same order, so the
// distances are the untyped kernel's bits); the ids sit in LDS, two buffers deep -- a slower wave may still select on the previous
// tile's -- and thread tl < 64 requests the NEXT tile's id a tile ahead, so the load flies under the distances.  Row liveness (the
// entity a member of the query-side set of r), the filter cursor at the tile's first id and the gathered tile's filter are the
// DistMult kernel's.
struct TeEntityTopkTypedParams {
    TeEntityTopkParams e;         // span_tiles / n_spans count tiles of the member lists
    TopkTyped ty;
};

template <int NK>
__global__ __launch_bounds__(256) void k_transe_entity_topk_typed_span(const TeEntityTopkTypedParams pp) {
    __shared__ __attribute__((aligned(16))) float qs[TE_KC][TE_TQ + 4];
    __shared__ __attribute__((aligned(16))) float es[TE_KC][TE_TE + 4];
    __shared__ __attribute__((aligned(16))) float ds[TE_TQ * TE_LDD];     // the tile's distances, row-major
    __shared__ unsigned long long thr[TE_TQ];
    __shared__ int cur[TE_TQ], fhi[TE_TQ], nxt[TE_TQ];
    __shared__ int fl[4][64];
    __shared__ int ent_s[TE_TQ];                                          // the rows' entities (-1: no such row)
    __shared__ int live_s[TE_TQ];                                         // the row's entity is on the query side of the relation at hand
    __shared__ int ids_s[2][TE_TE];                                       // the member ids of the tile at hand and of the previous one
    extern __shared__ unsigned long long lists[];                         // [TE_TQ][topk]
    const TeEntityTopkParams& tp = pp.e;
    const TopkTyped& ty = pp.ty;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, tx = tid & 15, ty4 = tid >> 4;
    const int k = tp.topk, dim = tp.dim, num_rels = tp.num_rels;
    const int m0 = blockIdx.x * TE_TQ;
    const int t_begin = blockIdx.y * tp.span_tiles;
    const int t_end = min(t_begin + tp.span_tiles, ty.n_tiles);
    const bool filtered = tp.filt_lo != nullptr, head = tp.head != 0;
    TopkTypedTile tile{};
    int my_id = -1;                                                       // thread tl < 64: slot tl of the tile about to be staged
    if (t_begin < t_end) {
        tile = topk_typed_seek(ty, num_rels, t_begin);
        if (tid < TE_TE) my_id = topk_typed_id(ty, tile, tp.n, tid);
    }
    topk_span_clear<TE_TQ>(lists, k, fl, thr, lane, wid, [&](int rl) { topk_pair_entity(tp.ents, m0, rl, tp.m, tp.n, ent_s); });
    int buf = 0;
    for (int t = t_begin; t < t_end; ++t) {
        // this buffer was last read by the selection two tiles back, which every wave left before this wave passed the previous
        // tile's barriers; te_tile_gather's first barrier publishes it (and the set-up above)
        int* ids = ids_s[buf];
        if (tid < TE_TE) ids[tid] = my_id;
        TopkTypedTile next = tile;
        if (t + 1 < t_end) {
            next = topk_typed_next(ty, num_rels, tile, t);
            if (tid < TE_TE) my_id = topk_typed_id(ty, next, tp.n, tid);
        }
        const float* __restrict__ rr = tp.rn + (size_t)tile.r * dim;
        float acc[4][4];
        te_tile_gather(
            [&](int row, int c) {
                const int a = ent_s[row];
                if (a < 0 || c >= dim) return 0.f;
                const float x = tp.en[(size_t)a * dim + c], y = rr[c];
                return head ? x - y : x + y;
            },
            [&](int row, int c) {
                const int id = ids[row];
                return (id >= 0 && c < dim) ? tp.en[(size_t)id * dim + c] : 0.f;
            },
            dim, tp.p, qs, es, acc);
        // (every wave is past the tile's last barrier: nobody still reads the previous relation's cursors or flags)
        if ((tile.ct == 0 || t == t_begin) && tid < TE_TQ) {
            const int a = ent_s[tid];
            const bool live = a >= 0 && topk_typed_member(ty, num_rels, tile.r, a);
            live_s[tid] = live;
            topk_filter_begin(tp.filt_lo, tp.filt_hi, tp.filt_ent, tp.n_ent, filtered && live, (long long)a * num_rels + tile.r,
                              max(ids[0], 0), &cur[tid], &fhi[tid], &nxt[tid]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
            *reinterpret_cast<float4*>(&ds[(4 * ty4 + a) * TE_LDD + 4 * tx]) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        __syncthreads();
        const int cnt = max(tile.live(), 1);
        const int x = ids[lane], id_max = ids[cnt - 1];
        topk_span_select<NK, TE_TQ>(m0, tp.m, lists, thr, k, lane, wid, [&](int rl, int) {
            const int a = ent_s[rl];
            unsigned long long key = x >= 0 ? topk_key(-ds[rl * TE_LDD + lane], tile.r * tp.n + x) : 0ull;
            if (filtered && nxt[rl] <= id_max &&
                topk_typed_filter_window(tp.filt_ent, ids, cnt, id_max, (int)((unsigned)(t - t_begin) * TE_TQ + rl + 1u), lane, &cur[rl],
                                         &fhi[rl], &nxt[rl], fl[wid]))
                key = 0ull;
            return tp.exclude_self && x == a ? 0ull : key;
        }, [&](int rl) { return live_s[rl] != 0; });
        tile = next;
        buf ^= 1;
    }
    if (t_begin >= t_end) __syncthreads();                                // a span without a tile: the set-up's lists, published
    topk_span_hand_on<TE_TQ>(m0, tp.m, lists, k, tp.part, tp.n_spans, lane, wid);
}

// ---- relation prediction (gv_transe_pair_rel): the query is an entity pair, the candidates are the relations ---------------------
// d[i, r] = ||(en[o_i] - en[s_i]) - rn[r]||_p: k_pair_rel (k_gemm.hip) on distances.  The query row en[o] - en[s], one f32
// subtraction per element, is formed while te_tile_with stages it, and the relation table is the tile's "entity" side, so a
// distance is gv_transe_distances' bits for that row against rn.  In exact arithmetic this is ||n(s) + n(r) - n(o)||, the triplet's
// distance; it is NOT the bit pattern k_transe_topk_span reports for the same triplet, whose query row is (n(s) + n(r)) and whose
// difference is taken against n(o): the operands are associated differently, each form rounds once where the other does not.
// Nothing compares the two.  L2 stays on the vector ALU like every distance here (no MFMA route: DESIGN.md 4c).
// One workgroup owns 64 pairs and walks all ceil(R / 64) relation tiles in ascending order: no spans, no workspace, no merge.  The
// target's distance is a tile's own element: with one relation tile it is read back from ds; with more, one extra tile is made ahead
// of the walk with the relation rows GATHERED through the rows' targets (te_tile_gather: the same staging, the same column order,
// the same per-pair chain) and its element (j, j) is row j's.  Counts and lists live in LDS and belong to the wave that owns the
// row; nothing is atomic.
// CAND (gv_transe_pair_rel_constrained): k_pair_rel<., CAND>'s sets -- the AND of two rows of the relation bitmask, fetched by
// thread rl < 64 once per tile after the tile's distances are made (TopkPairCand, k_topk.h) -- add the two counts among the
// type-correct relations and narrow the list; distances, raw and filtered counts are the unconstrained kernel's, whose code stays.
struct TePairRelParams {
    const float* en;              // [n, dim]
    const float* rn;              // [num_rels, dim]
    const int32_t* s;             // [m] the pairs' entities, trusted to lie in [0, n)
    const int32_t* o;
    const int32_t* target;        // NULL: no ranks
    const int32_t* filt_lo;       // NULL: no filter
    const int32_t* filt_hi;
    const int32_t* filt_rel;
    int m, num_rels, dim, p;
    int n_filt;                   // length of filt_rel: every range is clamped into it
    int topk;                     // 0: no list
    float* tgt;
    int32_t* count_raw;           // may be NULL
    int32_t* count_filt;          // NULL without a filter
    int64_t* out_ids;
    float* out_dist;
};

struct TePairRelCParams {
    TePairRelParams t;
    TopkPairCand cs;
    int32_t* count_raw_c;         // may be NULL
    int32_t* count_filt_c;        // NULL without a filter
};

__device__ __forceinline__ const TePairRelParams& te_pair_rel_params(const TePairRelParams& tp) { return tp; }
__device__ __forceinline__ const TePairRelParams& te_pair_rel_params(const TePairRelCParams& tc) { return tc.t; }

// k_transe_rank's predicates: nearer, or either side NaN; the key of gv_transe_topk
struct TePairRelRule {
    static __device__ __forceinline__ bool above(float d, float t) { return !(d >= t); }
    static __device__ __forceinline__ unsigned long long key(float d, int col) { return topk_key(-d, col); }
};

template <int NK, bool CAND = false>      // NK: keys per lane of a row's list: 0 (ranks only), 1 (k <= 64), 2
__global__ __launch_bounds__(256) void k_transe_pair_rel(const std::conditional_t<CAND, TePairRelCParams, TePairRelParams> tq) {
    const TePairRelParams& tp = te_pair_rel_params(tq);
    __shared__ __attribute__((aligned(16))) float qs[TE_KC][TE_TQ + 4];
    __shared__ __attribute__((aligned(16))) float es[TE_KC][TE_TE + 4];
    __shared__ __attribute__((aligned(16))) float ds[TE_TQ * TE_LDD];     // the tile's distances, row-major
    __shared__ unsigned long long thr[TE_TQ];                             // each row's k-th key
    __shared__ int cur[TE_TQ], fhi[TE_TQ], nxt[TE_TQ];                    // filter cursor (k_topk.h)
    __shared__ int fl[4][64];
    __shared__ int s_s[TE_TQ], o_s[TE_TQ];                                // the rows' pairs (-1: no such row)
    __shared__ int tcol_s[TE_TQ];                                         // the rows' targets (-1: none)
    __shared__ float dt_s[TE_TQ];                                         // ... and their distances
    __shared__ int cnt_s[CAND ? 4 : 2][TE_TQ];                            // 2 #better + #equal: raw, filtered (CAND: + among the allowed)
    __shared__ unsigned long long allow_s[CAND ? TE_TQ : 1];              // CAND: the rows' allowed relations of the tile at hand
    extern __shared__ unsigned long long lists[];                         // [TE_TQ][topk]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, tx = tid & 15, ty = tid >> 4;
    const int k = tp.topk, dim = tp.dim;
    const int m0 = blockIdx.x * TE_TQ;
    const int col_tiles = (tp.num_rels + TE_TE - 1) / TE_TE;
    const bool filtered = tp.filt_lo != nullptr, ranked = tp.target != nullptr;
    const TopkPairRel st{lists, thr, cur, fhi, nxt, fl, tcol_s, dt_s, cnt_s, allow_s};
    if constexpr (NK > 0)
        for (int i = tid; i < TE_TQ * k; i += 256) lists[i] = 0ull;
    fl[wid][lane] = 0;
    if (tid < TE_TQ) {
        const int row = m0 + tid;
        const bool live = row < tp.m;
        const int a = live ? tp.s[row] : -1, b = live ? tp.o[row] : -1;
        const int tc = (ranked && live) ? tp.target[row] : -1;
        s_s[tid] = a; o_s[tid] = b; tcol_s[tid] = tc;
        thr[tid] = 0ull;
        cnt_s[0][tid] = 0; cnt_s[1][tid] = 0;
        if constexpr (CAND) { cnt_s[2][tid] = 0; cnt_s[3][tid] = 0; }
        dt_s[tid] = __uint_as_float(0x7fc00000u);                         // a target outside [0, R) ranks last
        topk_filter_begin(tp.filt_lo, tp.filt_hi, tp.filt_rel, tp.n_filt, filtered && live, row, 0, &cur[tid], &fhi[tid], &nxt[tid]);
    }
    auto q_at = [&](int row, int c) {
        const int a = s_s[row];
        if (a < 0 || c >= dim) return 0.f;
        return tp.en[(size_t)o_s[row] * dim + c] - tp.en[(size_t)a * dim + c];
    };
    if (ranked && col_tiles > 1) {                 // the targets' distances: ONE gathered tile whose column j is rn[target of row j]
        float acc[4][4];
        te_tile_gather(                            // (its first barrier publishes the set-up above)
            q_at,
            [&](int row, int c) {
                const int tc = tcol_s[row];
                return ((unsigned)tc < (unsigned)tp.num_rels && c < dim) ? tp.rn[(size_t)tc * dim + c] : 0.f;
            },
            dim, tp.p, qs, es, acc);
        if (tx == ty) {                            // element (j, j) is row j's own
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if ((unsigned)tcol_s[4 * ty + a] < (unsigned)tp.num_rels) dt_s[4 * ty + a] = acc[a][a];
        }
    }
    for (int t = 0; t < col_tiles; ++t) {
        const int e0 = t * TE_TE;
        float acc[4][4];
        // te_tile_with's first barrier publishes the set-up above (and the gathered tile's dt_s) and ends the last tile's reads of ds
        te_tile_with(q_at, tp.rn, tp.num_rels, dim, tp.p, e0, qs, es, acc);
        if constexpr (CAND)                        // (every wave is past the tile's first barrier: nobody still reads the last tile's)
            if (tid < TE_TQ) allow_s[tid] = topk_pair_rel_allow(tq.cs, s_s[tid], o_s[tid], e0, tp.num_rels);
#pragma unroll
        for (int a = 0; a < 4; ++a)
            *reinterpret_cast<float4*>(&ds[(4 * ty + a) * TE_LDD + 4 * tx]) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        __syncthreads();
        if (ranked && col_tiles == 1) {            // the one tile holds every target
            if (tid < TE_TQ && (unsigned)tcol_s[tid] < (unsigned)tp.num_rels) dt_s[tid] = ds[tid * TE_LDD + tcol_s[tid]];
            __syncthreads();
        }
        topk_pair_rel_tile<NK, TePairRelRule, CAND>(st, m0, tp.m, e0, tp.num_rels, t, k, ranked, tp.filt_rel, lane, wid,
                                                    [&](int rl) { return ds[rl * TE_LDD + lane]; });
    }
    if constexpr (CAND)
        topk_pair_rel_store<NK, int64_t, te_key_dist, true>(st, m0, tp.m, k, ranked, tp.tgt, tp.count_raw, tp.count_filt, tp.out_ids,
                                                            tp.out_dist, lane, wid, tq.count_raw_c, tq.count_filt_c);
    else
        topk_pair_rel_store<NK, int64_t, te_key_dist>(st, m0, tp.m, k, ranked, tp.tgt, tp.count_raw, tp.count_filt, tp.out_ids,
                                                      tp.out_dist, lane, wid);
}

}  // namespace gv

using namespace gv;

extern "C" int gv_transe_sample(const uint64_t* rng_state, uint32_t stream, const int32_t* train, int64_t n_train, int n_ent,
                                const float* p_head, const int32_t* f_lo, const int32_t* f_hi, const int32_t* f_ent_o,
                                const int32_t* f_ent_s, int batch, int neg_ent, int32_t* bh, int32_t* br, int32_t* bt,
                                uint32_t* draws, void* stream_) {
    GV_REQUIRE(n_train > 0 && n_train < (1ll << 31) && n_ent > 0 && batch > 0 && neg_ent >= 0, GV_ERR_SHAPE,
               "gv_transe_sample: n_train=%lld n_ent=%d batch=%d neg_ent=%d", (long long)n_train, n_ent, batch, neg_ent);
    GV_REQUIRE((int64_t)batch * (1 + neg_ent) < (1ll << 31), GV_ERR_SHAPE, "gv_transe_sample: batch * (1 + neg_ent) >= 2^31");
    GV_REQUIRE(rng_state && train && bh && br && bt, GV_ERR_NULL, "gv_transe_sample: NULL pointer");
    GV_REQUIRE(!f_lo || (f_hi && f_ent_o && f_ent_s), GV_ERR_NULL, "gv_transe_sample: a filter needs f_lo, f_hi, f_ent_o, f_ent_s");
    hipLaunchKernelGGL(k_transe_sample, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream_, rng_state, stream, train,
                       n_train, n_ent, p_head, f_lo, f_hi, f_ent_o, f_ent_s, batch, neg_ent, bh, br, bt, draws);
    return launch_status("gv_transe_sample");
}

extern "C" int gv_transe_step(const float* ent, const float* rel, const int32_t* bh, const int32_t* br, const int32_t* bt, int batch,
                              int neg_ent, int dim, int p_norm, int norm_flag, float margin, float adv_temperature, float regul_rate,
                              float* g_ent, float* g_rel, float* loss_part, float* score, int32_t* occ_ent, void* stream) {
    GV_REQUIRE(batch > 0 && neg_ent > 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2), GV_ERR_SHAPE,
               "gv_transe_step: batch=%d neg_ent=%d dim=%d (1..%d) p_norm=%d (1 or 2)", batch, neg_ent, dim, GV_TRANSE_MAX_DIM, p_norm);
    GV_REQUIRE((int64_t)batch * (2 + neg_ent) * dim < (1ll << 40), GV_ERR_SHAPE, "gv_transe_step: batch too large");
    GV_REQUIRE(ent && rel && bh && br && bt && g_ent && g_rel && loss_part, GV_ERR_NULL, "gv_transe_step: NULL pointer");
    TeStepArgs a{ent, rel, bh, br, bt, batch, neg_ent, dim, p_norm, norm_flag, margin, adv_temperature, regul_rate,
                 g_ent, g_rel, loss_part, score, occ_ent};
    hipLaunchKernelGGL(k_transe_step, dim3((batch + 3) / 4), dim3(256), 0, GV_ST, a);
    return launch_status("gv_transe_step");
}

extern "C" int gv_transe_apply(float* ent, int n_ent, const float* g_ent, const int32_t* perm_e, const int32_t* rowptr_e, float* rel,
                               int n_rel, const float* g_rel, const int32_t* perm_r, const int32_t* rowptr_r, int dim, float lr,
                               const float* loss_part, int batch, float margin, float* loss_out, double* epoch_acc, void* stream) {
    GV_REQUIRE(n_ent > 0 && n_rel > 0 && dim > 0 && batch > 0, GV_ERR_SHAPE, "gv_transe_apply: n_ent=%d n_rel=%d dim=%d batch=%d",
               n_ent, n_rel, dim, batch);
    GV_REQUIRE(ent && g_ent && perm_e && rowptr_e && rel && g_rel && perm_r && rowptr_r && loss_part && loss_out, GV_ERR_NULL,
               "gv_transe_apply: NULL pointer");
    const int row_blocks = (int)(((int64_t)n_ent + n_rel + 3) / 4);
    hipLaunchKernelGGL(k_transe_apply, dim3(row_blocks + 1), dim3(256), 0, GV_ST, ent, n_ent, g_ent, perm_e, rowptr_e, rel, n_rel,
                       g_rel, perm_r, rowptr_r, dim, lr, loss_part, batch, margin, loss_out, epoch_acc, row_blocks);
    return launch_status("gv_transe_apply");
}

extern "C" int gv_transe_apply_opt(float* ent, int n_ent, const float* g_ent, const int32_t* perm_e, const int32_t* rowptr_e,
                                   float* rel, int n_rel, const float* g_rel, const int32_t* perm_r, const int32_t* rowptr_r, int dim,
                                   int method, double lr, double weight_decay, double lr_decay, float* s1_ent, float* s2_ent,
                                   float* s1_rel, float* s2_rel, const int64_t* step_t, const float* loss_part, int batch,
                                   float margin, float* loss_out, double* epoch_acc, void* stream) {
    GV_REQUIRE(n_ent > 0 && n_rel > 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM && batch > 0 && (int64_t)n_ent + n_rel < (1ll << 31) - 4,
               GV_ERR_SHAPE, "gv_transe_apply_opt: n_ent=%d n_rel=%d dim=%d (1..%d) batch=%d", n_ent, n_rel, dim, GV_TRANSE_MAX_DIM, batch);
    GV_REQUIRE(method >= GV_TRANSE_OPT_SGD && method <= GV_TRANSE_OPT_ADAM, GV_ERR_SHAPE,
               "gv_transe_apply_opt: method=%d (0 sgd, 1 adagrad, 2 adadelta, 3 adam)", method);
    GV_REQUIRE(lr >= 0.0 && weight_decay >= 0.0 && lr_decay >= 0.0, GV_ERR_SHAPE,
               "gv_transe_apply_opt: lr=%g weight_decay=%g lr_decay=%g must all be >= 0", lr, weight_decay, lr_decay);
    GV_REQUIRE(ent && g_ent && perm_e && rowptr_e && rel && g_rel && perm_r && rowptr_r && loss_part && loss_out, GV_ERR_NULL,
               "gv_transe_apply_opt: NULL pointer");
    GV_REQUIRE(method == GV_TRANSE_OPT_SGD || (s1_ent && s1_rel), GV_ERR_NULL, "gv_transe_apply_opt: method %d needs s1_ent and s1_rel",
               method);
    GV_REQUIRE(method < GV_TRANSE_OPT_ADADELTA || (s2_ent && s2_rel), GV_ERR_NULL,
               "gv_transe_apply_opt: method %d needs s2_ent and s2_rel", method);
    GV_REQUIRE((method != GV_TRANSE_OPT_ADAGRAD && method != GV_TRANSE_OPT_ADAM) || step_t, GV_ERR_NULL,
               "gv_transe_apply_opt: method %d needs step_t", method);
    const int row_blocks = (int)(((int64_t)n_ent + n_rel + 3) / 4);
    TeOptArgs a{ent, rel, s1_ent, s2_ent, s1_rel, s2_rel, g_ent, g_rel, perm_e, rowptr_e, perm_r, rowptr_r, step_t, loss_part, loss_out,
                epoch_acc, lr, weight_decay, lr_decay, n_ent, n_rel, dim, method, batch, row_blocks, margin};
    hipLaunchKernelGGL(k_transe_apply_opt, dim3(row_blocks + 1), dim3(256), 0, GV_ST, a);
    return launch_status("gv_transe_apply_opt");
}

extern "C" int gv_transe_queries(const float* ent, const float* rel, const int32_t* a, const int32_t* r, int64_t m, int dim,
                                 int head, int norm_flag, float* q, void* stream) {
    GV_REQUIRE(m >= 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM, GV_ERR_SHAPE, "gv_transe_queries: m=%lld dim=%d (1..%d)", (long long)m,
               dim, GV_TRANSE_MAX_DIM);
    if (m == 0) return GV_OK;
    GV_REQUIRE(ent && q && (!rel || (a && r)), GV_ERR_NULL, "gv_transe_queries: NULL pointer");
    hipLaunchKernelGGL(k_transe_queries, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, GV_ST, ent, rel, a, r, m, dim, head, norm_flag, q);
    return launch_status("gv_transe_queries");
}

extern "C" int gv_transe_distances(const float* q, int64_t m, const float* en, int v, int dim, int p_norm, float* out, void* stream) {
    GV_REQUIRE(m >= 0 && m < (1ll << 31) && v > 0 && dim > 0 && (p_norm == 1 || p_norm == 2), GV_ERR_SHAPE,
               "gv_transe_distances: m=%lld v=%d dim=%d p_norm=%d", (long long)m, v, dim, p_norm);
    if (m == 0) return GV_OK;
    GV_REQUIRE(q && en && out, GV_ERR_NULL, "gv_transe_distances: NULL pointer");
    hipLaunchKernelGGL(k_transe_distances, dim3((unsigned)((m + TE_TQ - 1) / TE_TQ), (unsigned)((v + TE_TE - 1) / TE_TE)), dim3(256),
                       0, GV_ST, q, m, en, v, dim, p_norm, out);
    return launch_status("gv_transe_distances");
}

// gv_transe_rank_filtered, and with cs.cand its type-constrained form
static int transe_rank_any(const char* name, const float* q, int64_t m, const float* en, int v, int dim, int p_norm, const int32_t* target,
                           const int32_t* f_lo, const int32_t* f_hi, const int32_t* f_ent, const TopkCand& cs, int32_t* counts_raw,
                           int32_t* counts_filt, int32_t* counts_raw_c, int32_t* counts_filt_c, void* stream) {
    hipError_t e = hipSuccess;
    for (int32_t* c : {counts_raw, counts_filt, counts_raw_c, counts_filt_c})
        if (c && e == hipSuccess) e = fill_words(c, 0u, (size_t)m * 4, GV_ST);
    GV_REQUIRE(e == hipSuccess, (int)e, "%s: clearing the counts: %s", name, hipGetErrorString(e));
    const int64_t q_tiles = (m + TE_TQ - 1) / TE_TQ;
    const int e_tiles = (v + TE_TE - 1) / TE_TE;
    int64_t split = (4 * (int64_t)current_device_cus() + q_tiles - 1) / q_tiles;
    if (split > e_tiles) split = e_tiles;
    if (split < 1) split = 1;
    const dim3 grid((unsigned)q_tiles, (unsigned)split), block(256);
    if (cs.cand)
        hipLaunchKernelGGL(k_transe_rank<true>, grid, block, 0, GV_ST, q, m, en, v, dim, p_norm, target, f_lo, f_hi, f_ent, counts_raw,
                           counts_filt, cs, counts_raw_c, counts_filt_c);
    else
        hipLaunchKernelGGL(k_transe_rank<false>, grid, block, 0, GV_ST, q, m, en, v, dim, p_norm, target, f_lo, f_hi, f_ent, counts_raw,
                           counts_filt, cs, counts_raw_c, counts_filt_c);
    return launch_status(name);
}

static int transe_rank_sizes(const char* name, int64_t m, int v, int dim, int p_norm) {
    GV_REQUIRE(m >= 0 && m < (1ll << 31) && v > 0 && dim > 0 && (p_norm == 1 || p_norm == 2), GV_ERR_SHAPE,
               "%s: m=%lld v=%d dim=%d p_norm=%d", name, (long long)m, v, dim, p_norm);
    return GV_OK;
}

extern "C" int gv_transe_rank_filtered(const float* q, int64_t m, const float* en, int v, int dim, int p_norm, const int32_t* target,
                                       const int32_t* f_lo, const int32_t* f_hi, const int32_t* f_ent, int32_t* counts_raw,
                                       int32_t* counts_filt, void* stream) {
    const char* name = "gv_transe_rank_filtered";
    GV_CHECK(transe_rank_sizes(name, m, v, dim, p_norm));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && en && target && counts_raw && counts_filt));
    GV_CHECK(query_filter_needs(name, f_lo, f_hi && f_ent, "f_lo, f_hi and f_ent"));
    return transe_rank_any(name, q, m, en, v, dim, p_norm, target, f_lo, f_hi, f_ent, TopkCand{}, counts_raw, counts_filt, nullptr,
                           nullptr, stream);
}

extern "C" int gv_transe_rank_constrained(const float* q, int64_t m, const float* en, int v, int dim, int p_norm, const int32_t* target,
                                          const int32_t* f_lo, const int32_t* f_hi, const int32_t* f_ent, const uint32_t* cand,
                                          int ld_cand, int n_sets, const int32_t* cand_set, int32_t* counts_raw, int32_t* counts_filt,
                                          int32_t* counts_raw_c, int32_t* counts_filt_c, void* stream) {
    const char* name = "gv_transe_rank_constrained";
    GV_CHECK(transe_rank_sizes(name, m, v, dim, p_norm));
    GV_CHECK(query_cand_shape(name, n_sets, ld_cand, v));
    GV_CHECK(query_filter(name, f_lo, f_hi, f_ent, "f_lo / f_hi / f_ent"));
    GV_CHECK(query_cand_given(name, cand, cand_set));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && en && target && counts_raw && counts_raw_c));
    GV_CHECK(query_filter_needs(name, f_lo, counts_filt && counts_filt_c, "both filtered counts"));
    const bool f = f_lo != nullptr;           // without a filter the two filtered counts are not written
    return transe_rank_any(name, q, m, en, v, dim, p_norm, target, f_lo, f_hi, f_ent, TopkCand{cand, cand_set, ld_cand, n_sets},
                           counts_raw, f ? counts_filt : nullptr, counts_raw_c, f ? counts_filt_c : nullptr, stream);
}

extern "C" int64_t gv_transe_topk_workspace_bytes(int64_t m, int v, int k) {
    if (m <= 0 || m >= (1ll << 31) || v <= 0 || k < 1 || k > TOPK_MAX) return 0;
    int span_tiles = 0, n_spans = 0;
    topk_spans(m, v, &span_tiles, &n_spans);
    return m * n_spans * k * (int64_t)sizeof(unsigned long long);
}

static int transe_topk_sizes(const char* name, int64_t m, int v, int dim, int p_norm, int n_filt_ent) {
    GV_REQUIRE(m >= 0 && m < (1ll << 31) && v > 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2) &&
                   n_filt_ent >= 0,
               GV_ERR_SHAPE, "%s: m=%lld v=%d dim=%d (1..%d) p_norm=%d (1 or 2) n_filt_ent=%d", name, (long long)m, v, dim,
               GV_TRANSE_MAX_DIM, p_norm, n_filt_ent);
    return GV_OK;
}

// the launches of gv_transe_topk, and with cs.cand of its type-constrained form (the running lists: <= 64 KiB of LDS beside 36 KiB
// static, so the limit is raised for either NK)
template <bool CAND>
static int transe_topk_launch(const char* name, const float* q, int64_t m, const float* en, int v, int dim, int p_norm,
                              const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent,
                              const TopkCand& cs, int k, int64_t* out_ids, float* out_dist, void* workspace, void* stream) {
    TeTopkParams tp{q, en, filt_lo, filt_hi, filt_ent, m, v, dim, p_norm, n_filt_ent, k, 0, 0, (unsigned long long*)workspace, cs};
    topk_spans(m, v, &tp.span_tiles, &tp.n_spans);
    return topk_span_merge<k_transe_topk_span<1, CAND>, k_transe_topk_span<2, CAND>, true, TE_TQ>(
        name, dim3((unsigned)((m + TE_TQ - 1) / TE_TQ), (unsigned)tp.n_spans), tp, tp.part, (int)m, tp.n_spans, k,
        TopkOut<int64_t, te_key_dist>{out_ids, out_dist}, GV_ST);
}

extern "C" int gv_transe_topk(const float* q, int64_t m, const float* en, int v, int dim, int p_norm, const int32_t* filt_lo,
                              const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int k, int64_t* out_ids,
                              float* out_dist, void* workspace, void* stream) {
    const char* name = "gv_transe_topk";
    GV_CHECK(transe_topk_sizes(name, m, v, dim, p_norm, n_filt_ent));
    GV_CHECK(query_k(name, k));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && en && out_ids && out_dist && workspace));
    return transe_topk_launch<false>(name, q, m, en, v, dim, p_norm, filt_lo, filt_hi, filt_ent, n_filt_ent, TopkCand{}, k, out_ids,
                                     out_dist, workspace, stream);
}

extern "C" int gv_transe_topk_constrained(const float* q, int64_t m, const float* en, int v, int dim, int p_norm,
                                          const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent,
                                          const uint32_t* cand, int ld_cand, int n_sets, const int32_t* cand_set, int k,
                                          int64_t* out_ids, float* out_dist, void* workspace, void* stream) {
    const char* name = "gv_transe_topk_constrained";
    GV_CHECK(transe_topk_sizes(name, m, v, dim, p_norm, n_filt_ent));
    GV_CHECK(query_k(name, k));
    GV_CHECK(query_cand_shape(name, n_sets, ld_cand, v));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    GV_CHECK(query_cand_given(name, cand, cand_set));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && en && out_ids && out_dist && workspace));
    return transe_topk_launch<true>(name, q, m, en, v, dim, p_norm, filt_lo, filt_hi, filt_ent, n_filt_ent,
                                    TopkCand{cand, cand_set, ld_cand, n_sets}, k, out_ids, out_dist, workspace, stream);
}

// ---- per-entity completion (gv_transe_entity_topk): gv_entity_topk_scores' geometry, entity_query_* of k_query_args.h ----------
static_assert(TE_TQ == 64 && TE_TE == 64, "the span helpers of k_topk.h and entity_query_spans count 64 x 64 tiles");

extern "C" int64_t gv_transe_entity_topk_workspace_bytes(int m, int n, int num_rels, int k, int span_tiles) {
    return entity_query_workspace_bytes(m, n, num_rels, k, span_tiles);
}

extern "C" int gv_transe_entity_topk(const int32_t* ents, int m, const float* en, const float* rn, int n, int num_rels, int dim, int head,
                                     int p_norm, const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent,
                                     int n_filt_ent, int exclude_self, int k, int span_tiles, int64_t* out_rel, int64_t* out_ent,
                                     float* out_dist, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* name = "gv_transe_entity_topk";
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2) && n_filt_ent >= 0,
               GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d dim=%d (1..%d) p_norm=%d (1 or 2) n_filt_ent=%d", name, m, n, num_rels, dim,
               GV_TRANSE_MAX_DIM, p_norm, n_filt_ent);
    GV_CHECK(entity_query_shape(name, n, num_rels, k, span_tiles));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, ents && en && rn && out_rel && out_ent && out_dist && workspace));
    TeEntityTopkParams tp{en, rn, ents, filt_lo, filt_hi, filt_ent, m, n, num_rels, dim, p_norm, head != 0, exclude_self != 0,
                          n_filt_ent, k, 0, 0, (unsigned long long*)workspace};
    entity_query_spans(m, n, num_rels, span_tiles, &tp.span_tiles, &tp.n_spans);
    GV_CHECK(entity_query_workspace(name, m, k, span_tiles, tp.n_spans, workspace_bytes));
    // (<= 64 KiB of lists beside 37 KiB static: the limit is raised for either NK)
    return topk_span_merge<k_transe_entity_topk_span<1>, k_transe_entity_topk_span<2>, true, TE_TQ>(
        name, dim3((unsigned)(((long long)m + TE_TQ - 1) / TE_TQ), (unsigned)tp.n_spans), tp, tp.part, m, tp.n_spans, k,
        TopkPairOut<int64_t, te_key_dist>{out_rel, out_ent, out_dist, n}, GV_ST);
}

// ---- per-entity completion among type-correct facts (gv_transe_entity_topk_typed): spans of the member lists' tiles ----------------
extern "C" int64_t gv_transe_entity_topk_typed_workspace_bytes(int m, int n_tiles, int k, int span_tiles) {
    return entity_typed_workspace_bytes(m, n_tiles, k, span_tiles);
}

extern "C" int gv_transe_entity_topk_typed(const int32_t* ents, int m, const float* en, const float* rn, int n, int num_rels, int dim,
                                           int head, int p_norm, const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent,
                                           int n_filt_ent, const int64_t* set_ptr, const int32_t* set_ids, const int32_t* tile_ptr,
                                           int n_tiles, int cand_base, int exclude_self, int k, int span_tiles, int64_t* out_rel,
                                           int64_t* out_ent, float* out_dist, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* name = "gv_transe_entity_topk_typed";
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2) && n_filt_ent >= 0,
               GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d dim=%d (1..%d) p_norm=%d (1 or 2) n_filt_ent=%d", name, m, n, num_rels, dim,
               GV_TRANSE_MAX_DIM, p_norm, n_filt_ent);
    GV_CHECK(entity_query_shape(name, n, num_rels, k, span_tiles));
    GV_CHECK(entity_typed_shape(name, num_rels, n_tiles, cand_base));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, ents && en && rn && out_rel && out_ent && out_dist && workspace));
    GV_CHECK(entity_typed_given(name, set_ptr, set_ids, tile_ptr, n_tiles));
    TeEntityTopkTypedParams pp{TeEntityTopkParams{en, rn, ents, filt_lo, filt_hi, filt_ent, m, n, num_rels, dim, p_norm, head != 0,
                                                  exclude_self != 0, n_filt_ent, k, 0, 0, (unsigned long long*)workspace},
                               TopkTyped{(const long long*)set_ptr, set_ids, tile_ptr, cand_base, n_tiles}};
    TeEntityTopkParams& tp = pp.e;
    entity_typed_spans(m, n_tiles, span_tiles, &tp.span_tiles, &tp.n_spans);
    GV_CHECK(entity_query_workspace(name, m, k, span_tiles, tp.n_spans, workspace_bytes));
    const TopkPairOut<int64_t, te_key_dist> out{out_rel, out_ent, out_dist, n};
    if (n_tiles == 0) return topk_all_padding(name, tp.part, m, k, out, GV_ST);
    // (<= 64 KiB of lists beside 38 KiB static: the limit is raised for either NK)
    return topk_span_merge<k_transe_entity_topk_typed_span<1>, k_transe_entity_topk_typed_span<2>, true, TE_TQ>(
        name, dim3((unsigned)(((long long)m + TE_TQ - 1) / TE_TQ), (unsigned)tp.n_spans), pp, tp.part, m, tp.n_spans, k, out, GV_ST);
}

// ---- relation prediction (gv_transe_pair_rel{,_constrained}): one launch, the checks of gv_pair_rel_scores{,_constrained} in
// their order
template <bool CAND>
static int te_pair_rel_entry(const char* name, const float* en, const float* rn, int n, int num_rels, int dim, int p_norm, const int32_t* s,
                             const int32_t* o, const int32_t* target, const int32_t* filt_lo, const int32_t* filt_hi,
                             const int32_t* filt_rel, int n_filt_rel, const uint32_t* cand, int ld_cand, int n_sets, int k, float* tgt,
                             int32_t* count_raw, int32_t* count_filt, int32_t* count_raw_c, int32_t* count_filt_c, int64_t* out_ids,
                             float* out_dist, int m, void* stream) {
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && dim > 0 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2) && n_filt_rel >= 0,
               GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d dim=%d (1..%d) p_norm=%d (1 or 2) n_filt_rel=%d", name, m, n, num_rels, dim,
               GV_TRANSE_MAX_DIM, p_norm, n_filt_rel);
    GV_CHECK(pair_query_asks(name, k, target));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_rel, "filt_lo / filt_hi / filt_rel"));
    if constexpr (CAND) GV_CHECK(pair_query_cand(name, cand, ld_cand, n_sets, n, num_rels));
    if (m == 0) return GV_OK;
    GV_CHECK(pair_query_given(name, en && rn && s && o, target, tgt, k, out_ids, out_dist, filt_lo, count_filt));
    if constexpr (CAND) GV_CHECK(pair_query_given_cand(name, target, filt_lo, count_filt_c));
    const TePairRelParams tp{en, rn, s, o, target, filt_lo, filt_hi, filt_rel, m, num_rels, dim, p_norm, n_filt_rel, k, tgt,
                             count_raw, filt_lo ? count_filt : nullptr, out_ids, out_dist};
    std::conditional_t<CAND, TePairRelCParams, TePairRelParams> tx;
    if constexpr (CAND) tx = TePairRelCParams{tp, TopkPairCand{cand, ld_cand, n}, count_raw_c, filt_lo ? count_filt_c : nullptr};
    else tx = tp;
    constexpr int KEY = (int)sizeof(unsigned long long);
    const dim3 grid((unsigned)(((long long)m + TE_TQ - 1) / TE_TQ)), block(256);
    static unsigned long long raised1 = 0, raised2 = 0;      // (<= 64 KiB of lists beside 38 KiB static: the limit is raised for either NK)
    if (k == 0) {
        hipLaunchKernelGGL((k_transe_pair_rel<0, CAND>), grid, block, 0, GV_ST, tx);
    } else if (k <= 64) {
        if (!raise_dynamic_lds((const void*)k_transe_pair_rel<1, CAND>, TE_TQ * 64 * KEY, raised1, name)) return GV_ERR_SHAPE;
        hipLaunchKernelGGL((k_transe_pair_rel<1, CAND>), grid, block, TE_TQ * k * KEY, GV_ST, tx);
    } else {
        if (!raise_dynamic_lds((const void*)k_transe_pair_rel<2, CAND>, TE_TQ * TOPK_MAX * KEY, raised2, name)) return GV_ERR_SHAPE;
        hipLaunchKernelGGL((k_transe_pair_rel<2, CAND>), grid, block, TE_TQ * k * KEY, GV_ST, tx);
    }
    return launch_status(name);
}

extern "C" int gv_transe_pair_rel(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm, const int32_t* s,
                                  const int32_t* o, const int32_t* target, const int32_t* filt_lo, const int32_t* filt_hi,
                                  const int32_t* filt_rel, int n_filt_rel, int k, float* tgt, int32_t* count_raw, int32_t* count_filt,
                                  int64_t* out_ids, float* out_dist, int m, void* stream) {
    return te_pair_rel_entry<false>("gv_transe_pair_rel", en, rn, n, num_rels, dim, p_norm, s, o, target, filt_lo, filt_hi, filt_rel,
                                    n_filt_rel, nullptr, 0, 0, k, tgt, count_raw, count_filt, nullptr, nullptr, out_ids, out_dist, m, stream);
}

extern "C" int gv_transe_pair_rel_constrained(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm, const int32_t* s,
                                              const int32_t* o, const int32_t* target, const int32_t* filt_lo, const int32_t* filt_hi,
                                              const int32_t* filt_rel, int n_filt_rel, const uint32_t* cand, int ld_cand, int n_sets,
                                              int k, float* tgt, int32_t* count_raw, int32_t* count_filt, int32_t* count_raw_c,
                                              int32_t* count_filt_c, int64_t* out_ids, float* out_dist, int m, void* stream) {
    return te_pair_rel_entry<true>("gv_transe_pair_rel_constrained", en, rn, n, num_rels, dim, p_norm, s, o, target, filt_lo, filt_hi,
                                   filt_rel, n_filt_rel, cand, ld_cand, n_sets, k, tgt, count_raw, count_filt, count_raw_c, count_filt_c,
                                   out_ids, out_dist, m, stream);
}
