// ltr_losses.hip -- standalone listwise-loss kernels (gfx950) + their C-ABI launchers.
//
// One slate group (64..1024 threads) per slate, slate state in LDS, forward and analytic backward in one
// pass.  Small slates share a 256-thread workgroup (4 slates at S <= 32), so a launch has B/4..B
// workgroups >> 256 CUs for any realistic batch.  These kernels are VALU/transcendental-bound
// (S^2 sigmoids per slate against 12*S bytes of HBM traffic), see DESIGN.md.
#include "../../include/ltr_mi355x.h"
#include "ltr_slate_losses.h"
#include <type_traits>

using namespace ltr;

namespace {

// ------------------------------------------------------------------------------------ approxNDCG
constexpr int kApproxArrays = 7;  // sc yl gn gg uu mk um
__global__ void __launch_bounds__(1024)
approxndcg_kernel(const float *__restrict__ scores, const float *__restrict__ labels, int B, int S, int group,
                  float alpha, float eps, float pad, float gscale, float *__restrict__ slate_loss,
                  float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3;
    const int gid = threadIdx.x / group;
    const long long slate = ltr_block_id() * (blockDim.x / group) + gid;
    const bool active = slate < B;
    float *base = smem + (size_t)gid * (kApproxArrays * s_al + group + 32);
    float *sc = base, *yl = sc + s_al, *gn = yl + s_al, *gg = gn + s_al, *uu = gg + s_al, *mk = uu + s_al;
    ApproxScratch xs;
    xs.um = mk + s_al;
    const SlateGroup g = make_group(S, group, xs.um + s_al);
    const size_t off = (size_t)slate * S;
    approx_ndcg_init(g);
    for (int j = g.t; j < S; j += group) {
        const float y = active ? labels[off + j] : pad;
        sc[j] = active ? scores[off + j] : 0.f;
        stage_label(y, pad, yl[j], gn[j]);
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    const float loss = approx_ndcg_slate(g, sc, yl, gn, gg, uu, mk, alpha, eps, gscale, dscores != nullptr,
                                         [&](int i, float v) { if (active) dst[i] = v; }, NoStamp(), xs);
    if (active && g.t == 0) slate_loss[slate] = loss;
}

// --------------------------------------------------------------------------------------- ListNet
__global__ void __launch_bounds__(1024)
listnet_kernel(const float *__restrict__ y_true, const float *__restrict__ y_pred, int B, int S, int group,
               int apply_sigmoid, float gscale, float *__restrict__ slate_loss, float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3;
    const int gid = threadIdx.x / group;
    const long long slate = ltr_block_id() * (blockDim.x / group) + gid;
    const bool active = slate < B;
    float *base = smem + (size_t)gid * (2 * s_al + group + 32);
    float *yt = base, *yp = yt + s_al;
    const SlateGroup g = make_group(S, group, yp + s_al);
    const size_t off = (size_t)slate * S;
    for (int j = g.t; j < S; j += group) {
        yt[j] = active ? y_true[off + j] : 0.f;
        yp[j] = active ? y_pred[off + j] : 0.f;
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    const float loss = listnet_slate(g, yt, yp, apply_sigmoid != 0, gscale, dscores != nullptr,
                                     [&](int i, float v) { if (active) dst[i] = v; });
    if (active && g.t == 0) slate_loss[slate] = loss;
}

// ------------------------------------------------------------------------------------ LambdaLoss
constexpr int kLambdaArrays = 7;  // sc yl gn w1 invd delta rk

__device__ __forceinline__ LambdaLds lambda_carve(float *base, int s_al) {
    LambdaLds L;
    L.sc = base;
    L.yl = L.sc + s_al;
    L.gn = L.yl + s_al;
    L.w1 = L.gn + s_al;
    L.invd = L.w1 + s_al;
    L.delta = L.invd + s_al;
    L.rk = reinterpret_cast<int *>(L.delta + s_al);
    return L;
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_kernel(const float *__restrict__ scores, const float *__restrict__ labels, int B, int S, int group,
              LambdaParams P, float pad, float gscale, float *__restrict__ slate_loss,
              float *__restrict__ slate_count, float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3;
    const int gid = threadIdx.x / group;
    const long long slate = ltr_block_id() * (blockDim.x / group) + gid;
    const bool active = slate < B;
    float *base = smem + (size_t)gid * (kLambdaArrays * s_al + group + 32);
    const LambdaLds L = lambda_carve(base, s_al);
    const SlateGroup g = make_group(S, group, base + kLambdaArrays * s_al);
    const size_t off = (size_t)slate * S;
    for (int j = g.t; j < S; j += group) {
        const float y = active ? labels[off + j] : pad;
        L.sc[j] = active ? scores[off + j] : 0.f;
        stage_label(y, pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    float count;
    const float loss = lambda_slate<SCH>(g, L, P, gscale, dscores != nullptr, &count,
                                         [&](int i, float v) { if (active) dst[i] = v; });
    if (active && g.t == 0) {
        slate_loss[slate] = loss;
        slate_count[slate] = count;
    }
}

// Long slates (256 <= S <= 1024, every scheme but ndcgLoss1): rank-space sweep, every unordered pair once
// (lambda_slate_blocked).  One slate per workgroup, one wave per 64 ranks.
template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_blocked_kernel(const float *__restrict__ scores, const float *__restrict__ labels, int B, int S, LambdaParams P,
                      float pad, float gscale, float *__restrict__ slate_loss, float *__restrict__ slate_count,
                      float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3, s64 = (S + 63) & ~63;
    const long long slate = ltr_block_id();
    if (slate >= B) return;                      // (whole block: the y-padding of a two-dimensional grid)
    const LambdaLds L = lambda_carve(smem, s_al);
    float *rb = smem + kLambdaArrays * s_al;
    LambdaRankLds R;
    R.rs = rb;
    R.ry = rb + s64;
    R.rg = rb + 2 * s64;
    R.colacc = rb + 3 * s64;
    R.doc_of = reinterpret_cast<int *>(rb + 4 * s64);
    const SlateGroup g = make_group(S, blockDim.x, rb + 5 * s64);
    const size_t off = (size_t)slate * S;
    for (int j = g.t; j < S; j += blockDim.x) {
        L.sc[j] = scores[off + j];
        stage_label(labels[off + j], pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    float count;
    const float loss = lambda_slate_blocked<SCH>(g, L, R, P, gscale, dscores != nullptr, &count,
                                                 [&](int i, float v) { dst[i] = v; });
    if (g.t == 0) {
        slate_loss[slate] = loss;
        slate_count[slate] = count;
    }
}

// Full pair matrix in predicted-rank order (lambdaMask(return_losses=True), lambdaL.py:49-60): every
// (ri, rj) including padded documents, whose score/label are -inf in the reference (:13-15):
//   d = clamp(s_i - s_j, +-1e8), NaN -> 0;  G = 0 and clamped label = 0 for padded documents.
template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_pairs_fwd_kernel(const float *__restrict__ scores, const float *__restrict__ labels, int B, int S,
                        int group, LambdaParams P, float pad, float *__restrict__ losses,
                        uint8_t *__restrict__ keep, int32_t *__restrict__ rank) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3;
    const long long slate = ltr_block_id();
    if (slate >= B) return;                      // (whole block: the y-padding of a two-dimensional grid)
    float *base = smem;
    const LambdaLds L = lambda_carve(base, s_al);
    int *dar = reinterpret_cast<int *>(base + kLambdaArrays * s_al);   // document at rank r
    const SlateGroup g = make_group(S, group, base + (kLambdaArrays + 1) * s_al);
    const size_t off = (size_t)slate * S;
    for (int j = g.t; j < S; j += group) {
        L.sc[j] = scores[off + j];
        stage_label(labels[off + j], pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    lambda_prepare(g, L, P);
    for (int j = g.t; j < S; j += group) {
        dar[L.rk[j]] = j;
        if (rank) rank[off + j] = L.rk[j];
    }
    __syncthreads();
    const size_t moff = (size_t)slate * S * S;
    for (int e = g.t; e < S * S; e += group) {
        const int ri = e / S, rj = e - ri * S;
        const int i = dar[ri], j = dar[rj];
        const bool pi = L.gn[i] < 0.f, pj = L.gn[j] < 0.f;
        const float si = pi ? -INFINITY : L.sc[i], sj = pj ? -INFINITY : L.sc[j];
        float d = si - sj;
        d = (d != d) ? 0.f : fminf(fmaxf(d, -1e8f), 1e8f);
        float u, um;
        sigmoid_pair(P.sigma * d, u, um);
        const float Gi = fmaxf(L.gn[i], 0.f), Gj = fmaxf(L.gn[j], 0.f);
        const float yci = fmaxf(L.yl[i], 0.f), ycj = fmaxf(L.yl[j], 0.f);
        float ell, dl;
        lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, L.rk[i], L.rk[j], L.invd[i], L.invd[j], L.w1[i], Gi, Gj, yci, ycj),
                         u, um, ell, dl);
        losses[moff + e] = ell;
        if (keep) {
            const bool ok = !pi && !pj && (P.k <= 0 || (ri < P.k && rj < P.k)) && (SCH == 1 || L.yl[i] > L.yl[j]);
            keep[moff + e] = ok ? 1 : 0;
        }
    }
}

// One term of a column sum, compensated (Kahan): a column of S near-equal terms (rankNet weights on tied scores: every term
// log_b(1/2)) summed naively in fp32 rounds the same way at every step and drifts by S ulp -- 1.5e-5 relative at S = 2048,
// past the 1e-5 parity bar.  The three column-sum kernels share this step, so they stay bitwise equal to each other.
__device__ __forceinline__ void colsum_add(float &acc, float &comp, float term) {
    const float yk = term - comp;
    const float tk = acc + yk;
    comp = (tk - acc) - yk;
    acc = tk;
}

// Column sums of the pair matrix, c[b, rj] = sum_ri losses[b, ri, rj] (what the risk losses take from
// lambdaMask(return_losses=True): torch.sum(..., dim=1), riskLosses.py:72-83) WITHOUT materialising [B,S,S].
template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_colsum_fwd_kernel(const float *__restrict__ scores, const float *__restrict__ labels, int B, int S,
                         int group, LambdaParams P, float pad, float *__restrict__ colsum) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3;
    const long long slate = ltr_block_id();
    if (slate >= B) return;                      // (whole block: the y-padding of a two-dimensional grid)
    float *base = smem;
    const LambdaLds L = lambda_carve(base, s_al);
    int *dar = reinterpret_cast<int *>(base + kLambdaArrays * s_al);   // document at rank r
    const SlateGroup g = make_group(S, group, base + (kLambdaArrays + 1) * s_al);
    const size_t off = (size_t)slate * S;
    for (int j = g.t; j < S; j += group) {
        L.sc[j] = scores[off + j];
        stage_label(labels[off + j], pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    lambda_prepare(g, L, P);
    for (int j = g.t; j < S; j += group) dar[L.rk[j]] = j;
    __syncthreads();
    for (int rj = g.t; rj < S; rj += group) {
        const int j = dar[rj];
        const bool pj = L.gn[j] < 0.f;
        const float sj = pj ? -INFINITY : L.sc[j];
        const float Gj = fmaxf(L.gn[j], 0.f), ycj = fmaxf(L.yl[j], 0.f);
        float acc = 0.f, comp = 0.f;
        for (int ri = 0; ri < S; ++ri) {          // rank order: the order torch.sum(dim=1) walks the column in
            const int i = dar[ri];
            const bool pi = L.gn[i] < 0.f;
            const float si = pi ? -INFINITY : L.sc[i];
            float d = si - sj;
            d = (d != d) ? 0.f : fminf(fmaxf(d, -1e8f), 1e8f);
            float u, um;
            sigmoid_pair(P.sigma * d, u, um);
            const float Gi = fmaxf(L.gn[i], 0.f), yci = fmaxf(L.yl[i], 0.f);
            float ell, dl;
            lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, L.rk[i], L.rk[j], L.invd[i], L.invd[j], L.w1[i], Gi, Gj, yci, ycj),
                             u, um, ell, dl);
            colsum_add(acc, comp, ell);
        }
        colsum[off + rj] = acc;
    }
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_pairs_bwd_kernel(const float *__restrict__ scores, const float *__restrict__ labels, int B, int S,
                        int group, LambdaParams P, float pad, const float *__restrict__ gup, int colsum,
                        float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_al = (S + 3) & ~3;
    const long long slate = ltr_block_id();
    if (slate >= B) return;                      // (whole block: the y-padding of a two-dimensional grid)
    float *base = smem;
    const LambdaLds L = lambda_carve(base, s_al);
    const SlateGroup g = make_group(S, group, base + kLambdaArrays * s_al);
    const size_t off = (size_t)slate * S;
    for (int j = g.t; j < S; j += group) {
        L.sc[j] = scores[off + j];
        stage_label(labels[off + j], pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    lambda_prepare(g, L, P);
    // colsum != 0: the upstream gradient is that of  c[b, rj] = sum_ri losses[b, ri, rj]  -> G[ri, rj] = gup[b, rj]
    const float *G = gup + (size_t)slate * S * (colsum ? 1 : S);
    for (int i0 = 0; i0 < S; i0 += g.sp) {
        const int i = i0 + g.ri;
        const bool row = i < S;
        const bool vi = row && L.gn[i] >= 0.f;
        float gr = 0.f;
        if (vi) {
            const float si = L.sc[i], Gi = L.gn[i], yci = fmaxf(L.yl[i], 0.f);
            const int ri = L.rk[i];
            for (int j = g.cg; j < S; j += g.CG) {
                const float Gj = L.gn[j];
                if (j == i || Gj < 0.f) continue;   // padded pairs sit in a clamped / NaN->0 region: no grad
                const int rj = L.rk[j];
                const float draw = si - L.sc[j];
                if (!(fabsf(draw) <= 1e8f)) continue;
                float u, um;
                sigmoid_pair(P.sigma * draw, u, um);
                const float ycj = fmaxf(L.yl[j], 0.f);
                float ell, dl_ij, dl_ji;
                lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, ri, rj, L.invd[i], L.invd[j], L.w1[i], Gi, Gj, yci, ycj),
                                 u, um, ell, dl_ij);
                lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, rj, ri, L.invd[j], L.invd[i], L.w1[j], Gj, Gi, ycj, yci),
                                 um, u, ell, dl_ji);
                const float g_ij = colsum ? G[rj] : G[(size_t)ri * S + rj];
                const float g_ji = colsum ? G[ri] : G[(size_t)rj * S + ri];
                gr += g_ij * dl_ij - g_ji * dl_ji;
            }
        }
        const float tot = row_reduce(g, gr);
        if (row && g.cg == 0) dscores[off + i] = vi ? P.sigma * tot : 0.f;
    }
}

// ---- Column sums for ALL systems of a Lambda-type risk loss in one launch (riskLosses.py:63-83, :183-203, :294-310): the reference
// soft-maxes labels, scores and every baseline over the slate (:65-70) and then takes torch.sum(lambdaMask(p, p_true, ...,
// return_losses=True), dim=1) once per system -- three softmax launches and three column-sum launches here until round 3.  One
// workgroup per (system, query): system 0 = the model, 1..n = the baselines, n + 1 = the ideal ranking (the labels as scores).
// v[0..S) -> softmax(v) in place (torch: exp(x - max) / sum); all threads of the block call (barriers inside)
__device__ __forceinline__ void slate_softmax(const SlateGroup &g, float *v, int S) {
    float m = -INFINITY;
    for (int j = g.t; j < S; j += g.group) m = fmaxf(m, v[j]);
    m = group_max(g, m);
    float z = 0.f;
    for (int j = g.t; j < S; j += g.group) {
        const float e = expf(v[j] - m);
        v[j] = e;
        z += e;
    }
    z = group_sum(g, z);
    for (int j = g.t; j < S; j += g.group) v[j] = v[j] / z;
    __syncthreads();
}

// One (system, slate): off = the slate's first document row, S its length, out = where its S column sums go.  Shared by the rectangular
// kernel and the ragged one (same group size -> same bits).
template <int SCH>
__device__ __forceinline__ void colsum_sys_slate(const float *__restrict__ y_pred, const float *__restrict__ y_true,
                                                 const float *__restrict__ y_base, const int sys, const size_t off, const int S, int nb,
                                                 int group, const LambdaParams &P, float pad, float *__restrict__ out, float *base) {
    const int s_al = (S + 3) & ~3;
    const LambdaLds L = lambda_carve(base, s_al);
    int *dar = reinterpret_cast<int *>(base + kLambdaArrays * s_al);   // document at rank r
    const SlateGroup g = make_group(S, group, base + (kLambdaArrays + 1) * s_al);
    for (int j = g.t; j < S; j += group) {
        L.yl[j] = y_true[off + j];
        L.sc[j] = sys == 0 ? y_pred[off + j] : (sys <= nb ? y_base[(off + j) * nb + (sys - 1)] : 0.f);
    }
    __syncthreads();
    slate_softmax(g, L.yl, S);
    if (sys <= nb) slate_softmax(g, L.sc, S);    // (block-uniform)
    for (int j = g.t; j < S; j += group) {
        const float pt = L.yl[j];
        if (sys > nb) L.sc[j] = pt;              // the ideal ranking scores the documents with the (soft-maxed) labels themselves
        stage_label(pt, pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    lambda_prepare(g, L, P);
    for (int j = g.t; j < S; j += group) dar[L.rk[j]] = j;
    __syncthreads();
    for (int rj = g.t; rj < S; rj += group) {
        const int j = dar[rj];
        const bool pj = L.gn[j] < 0.f;
        const float sj = pj ? -INFINITY : L.sc[j];
        const float Gj = fmaxf(L.gn[j], 0.f), ycj = fmaxf(L.yl[j], 0.f);
        float acc = 0.f, comp = 0.f;
        for (int ri = 0; ri < S; ++ri) {          // rank order: the order torch.sum(dim=1) walks the column in
            const int i = dar[ri];
            const bool pi = L.gn[i] < 0.f;
            const float si = pi ? -INFINITY : L.sc[i];
            float d = si - sj;
            d = (d != d) ? 0.f : fminf(fmaxf(d, -1e8f), 1e8f);
            float u, um;
            sigmoid_pair(P.sigma * d, u, um);
            const float Gi = fmaxf(L.gn[i], 0.f), yci = fmaxf(L.yl[i], 0.f);
            float ell, dl;
            lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, L.rk[i], L.rk[j], L.invd[i], L.invd[j], L.w1[i], Gi, Gj, yci, ycj),
                             u, um, ell, dl);
            colsum_add(acc, comp, ell);
        }
        out[rj] = acc;
    }
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_colsum_sys_fwd_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true, const float *__restrict__ y_base, int B,
                             int S, int nb, int group, LambdaParams P, float pad, float *__restrict__ colsum) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const long long blk = ltr_block_id();
    if (blk >= (long long)(nb + 2) * B) return;  // (whole block: the y-padding of a two-dimensional grid)
    const int sys = (int)(blk / B);
    const long long slate = blk - (long long)sys * B;
    colsum_sys_slate<SCH>(y_pred, y_true, y_base, sys, (size_t)slate * S, S, nb, group, P, pad,
                          colsum + ((size_t)sys * B + slate) * S, smem);
}

// ---- The Lambda-type risk step with the constant systems cached (ltr_mi355x.scorer.FusedRanker.baseline_columns): the baselines' and the
// ideal ranking's matrix entries and the ideal column sums depend on (y_true, y_base) only.  One workgroup per query runs the MODEL's
// column sums (slate softmaxes inside, as lambda_colsum_sys_fwd_kernel system 0), then its effectiveness against the cached ideal
// column sums and d mat[b][0] / d colsum (ltr_risk_matrix_fwd mode 1, column 0), and copies the cached entries into the row.
// Bitwise the same matrix as the two uncached launches: the column sums run with the same group size, and the effectiveness sums
// replay risk_matrix_kernel's 256-thread order (per-thread strides of 256, wave butterflies, four waves summed in order; with fewer
// than 256 threads S <= group, so the missing threads would have held zeros).
constexpr int kEffThreads = 256;

__device__ __forceinline__ double eff_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, LTR_WAVE);
    return v;
}
__device__ __forceinline__ double eff_block_sum(double v, double *red, int nw) {
    v = eff_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0 && threadIdx.x < kEffThreads) red[threadIdx.x / LTR_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kEffThreads / LTR_WAVE; ++w) s += w < nw ? red[w] : 0.0;
    return s;
}

// One slate: crow = its n_cached cached matrix entries, t = the ideal ranking's S column sums, mrow = its matrix row, off = its first
// document row.  Shared by the rectangular kernel and the ragged one.
template <int SCH>
__device__ __forceinline__ void risk_model_slate(const float *__restrict__ y_pred, const float *__restrict__ y_true,
                                                 const float *__restrict__ crow, const float *__restrict__ t, int n_cached,
                                                 const size_t off, const int S, int group,
                                                 const LambdaParams &P, float pad, int lt, float *__restrict__ mrow,
                                                 float *__restrict__ jac, float *base, double *red) {
    const int s_al = (S + 3) & ~3;
    const LambdaLds L = lambda_carve(base, s_al);
    int *dar = reinterpret_cast<int *>(base + kLambdaArrays * s_al);   // document at rank r
    float *x = base + (kLambdaArrays + 1) * s_al;                       // the model's column sums, by predicted rank
    const SlateGroup g = make_group(S, group, x + s_al);
    for (int k = threadIdx.x; k < n_cached; k += group) mrow[1 + k] = crow[k];
    for (int j = g.t; j < S; j += group) {
        L.yl[j] = y_true[off + j];
        L.sc[j] = y_pred[off + j];
    }
    __syncthreads();
    slate_softmax(g, L.yl, S);
    slate_softmax(g, L.sc, S);
    for (int j = g.t; j < S; j += group) stage_label(L.yl[j], pad, L.yl[j], L.gn[j]);
    __syncthreads();
    lambda_prepare(g, L, P);
    for (int j = g.t; j < S; j += group) dar[L.rk[j]] = j;
    __syncthreads();
    for (int rj = g.t; rj < S; rj += group) {
        const int j = dar[rj];
        const bool pj = L.gn[j] < 0.f;
        const float sj = pj ? -INFINITY : L.sc[j];
        const float Gj = fmaxf(L.gn[j], 0.f), ycj = fmaxf(L.yl[j], 0.f);
        float acc = 0.f, comp = 0.f;
        for (int ri = 0; ri < S; ++ri) {          // rank order: the order torch.sum(dim=1) walks the column in
            const int i = dar[ri];
            const bool pi = L.gn[i] < 0.f;
            const float si = pi ? -INFINITY : L.sc[i];
            float d = si - sj;
            d = (d != d) ? 0.f : fminf(fmaxf(d, -1e8f), 1e8f);
            float u, um;
            sigmoid_pair(P.sigma * d, u, um);
            const float Gi = fmaxf(L.gn[i], 0.f), yci = fmaxf(L.yl[i], 0.f);
            float ell, dl;
            lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, L.rk[i], L.rk[j], L.invd[i], L.invd[j], L.w1[i], Gi, Gj, yci, ycj),
                             u, um, ell, dl);
            colsum_add(acc, comp, ell);
        }
        x[rj] = acc;
    }
    __syncthreads();
    // effectiveness of the model against the ideal column sums (risk_matrix_kernel, mode 1, system 0)
    const int tid = threadIdx.x, nw = group / LTR_WAVE;
    const bool act = tid < kEffThreads;
    double nt_a = 0.0, st_a = 0.0;
    if (act)
        for (int j = tid; j < S; j += kEffThreads) {
            const float tj = t[j];
            nt_a += (double)tj * tj;
            st_a += (double)tj;
        }
    const double nt = eff_block_sum(nt_a, red, nw), st = eff_block_sum(st_a, red, nw);
    double a_a = 0.0, nx_a = 0.0, c_a = 0.0, sx_a = 0.0;
    if (act)
        for (int j = tid; j < S; j += kEffThreads) {
            const float tj = t[j], xj = x[j];
            a_a += (double)tj * xj;
            nx_a += (double)xj * xj;
            sx_a += (double)xj;
            const float df = xj - tj;
            c_a += (double)df * df;
        }
    const double a = eff_block_sum(a_a, red, nw), nx = eff_block_sum(nx_a, red, nw), c = eff_block_sum(c_a, red, nw),
                 sx = eff_block_sum(sx_a, red, nw);
    const double nrm_u = sqrt(nt), nrm_v = sqrt(nx);
    const double den = (nrm_u > 1e-8 ? nrm_u : 1e-8) * (nrm_v > 1e-8 ? nrm_v : 1e-8);
    double m;
    if (lt == 1) m = c;
    else if (lt == 2) m = a / den;
    else m = (sx - st) * (sx - st);
    if (tid == 0) mrow[0] = (float)m;
    const double nv_c = nrm_v > 1e-8 ? nrm_v : 1e-8;
    const double inv_vv = nrm_v > 0.0 ? 1.0 / (nv_c * nrm_v) : 0.0;
    for (int j = tid; j < S; j += group) {
        const double tj = t[j], xj = x[j];
        double gj;
        if (lt == 1) gj = 2.0 * (xj - tj);
        else if (lt == 2) gj = tj / den - m * xj * inv_vv;
        else gj = 2.0 * (sx - st);
        jac[off + j] = (float)gj;
    }
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_risk_model_fwd_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true, const float *__restrict__ cache,
                             int cache_stride, int n_cached, int B, int S, int group, LambdaParams P, float pad, int lt,
                             float *__restrict__ mat, float *__restrict__ jac) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kEffThreads / LTR_WAVE];
    const long long slate = ltr_block_id();
    if (slate >= B) return;                      // (whole block: the y-padding of a two-dimensional grid)
    const float *crow = cache + (size_t)slate * cache_stride;           // [n_cached matrix entries | ideal column sums [S]]
    risk_model_slate<SCH>(y_pred, y_true, crow, crow + n_cached, n_cached, (size_t)slate * S, S, group, P, pad, lt,
                          mat + (size_t)slate * (1 + n_cached), jac, smem, red);
}

// d L / d y_pred from d L / d colsum[system 0]: the pair backward on the soft-maxed vectors, then the softmax's Jacobian
// (d p_i / d s_k = p_i (delta_ik - p_k)):  ds_k = p_k (dp_k - sum_i p_i dp_i)
// One slate (off = its first document row, cq = its coefficient).  Shared by the rectangular kernel and the ragged one.
template <int SCH>
__device__ __forceinline__ void colsum_sys_bwd_slate(const float *__restrict__ y_pred, const float *__restrict__ y_true, const size_t off,
                                                     const int S, int group, const LambdaParams &P, float pad,
                                                     const float *__restrict__ gup, const float cq, float *__restrict__ dy_pred,
                                                     float *base) {
    const int s_al = (S + 3) & ~3;
    const LambdaLds L = lambda_carve(base, s_al);
    float *dp = base + kLambdaArrays * s_al;
    const SlateGroup g = make_group(S, group, dp + s_al);
    for (int j = g.t; j < S; j += group) {
        L.yl[j] = y_true[off + j];
        L.sc[j] = y_pred[off + j];
    }
    __syncthreads();
    slate_softmax(g, L.yl, S);
    slate_softmax(g, L.sc, S);
    for (int j = g.t; j < S; j += group) stage_label(L.yl[j], pad, L.yl[j], L.gn[j]);
    __syncthreads();
    lambda_prepare(g, L, P);
    const float *G = gup + off;
    for (int i0 = 0; i0 < S; i0 += g.sp) {
        const int i = i0 + g.ri;
        const bool row = i < S;
        const bool vi = row && L.gn[i] >= 0.f;
        float gr = 0.f;
        if (vi) {
            const float si = L.sc[i], Gi = L.gn[i], yci = fmaxf(L.yl[i], 0.f);
            const int ri = L.rk[i];
            for (int j = g.cg; j < S; j += g.CG) {
                const float Gj = L.gn[j];
                if (j == i || Gj < 0.f) continue;
                const int rj = L.rk[j];
                const float draw = si - L.sc[j];
                if (!(fabsf(draw) <= 1e8f)) continue;
                float u, um;
                sigmoid_pair(P.sigma * draw, u, um);
                const float ycj = fmaxf(L.yl[j], 0.f);
                float ell, dl_ij, dl_ji;
                lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, ri, rj, L.invd[i], L.invd[j], L.w1[i], Gi, Gj, yci, ycj),
                                 u, um, ell, dl_ij);
                lambda_pair_term(P, lambda_weight<SCH>(P, L.delta, rj, ri, L.invd[j], L.invd[i], L.w1[j], Gj, Gi, ycj, yci),
                                 um, u, ell, dl_ji);
                gr += (G[rj] * cq) * dl_ij - (G[ri] * cq) * dl_ji;
            }
        }
        const float tot = row_reduce(g, gr);
        if (row && g.cg == 0) dp[i] = vi ? P.sigma * tot : 0.f;
    }
    __syncthreads();
    float dot = 0.f;
    for (int j = g.t; j < S; j += group) dot += L.sc[j] * dp[j];
    dot = group_sum(g, dot);
    for (int j = g.t; j < S; j += group) dy_pred[off + j] = L.sc[j] * (dp[j] - dot);
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_colsum_sys_bwd_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true, int B, int S, int group, LambdaParams P,
                             float pad, const float *__restrict__ gup, const float *__restrict__ coef, int coef_stride,
                             float *__restrict__ dy_pred) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const long long slate = ltr_block_id();
    if (slate >= B) return;
    // coef != NULL: d L / d colsum[0] = gup (the Jacobian of the model's matrix entry) x coef[slate] (d L / d mat[slate][0])
    const float cq = coef ? coef[slate * coef_stride] : 1.f;
    colsum_sys_bwd_slate<SCH>(y_pred, y_true, (size_t)slate * S, S, group, P, pad, gup, cq, dy_pred, smem);
}

// --------------------------------------------------------------------------------------- ordinal
constexpr int kOrdBlock = 256;

__global__ void __launch_bounds__(kOrdBlock)
ordinal_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true, int64_t n_docs, int n,
               float pad, float *__restrict__ block_partials, float *__restrict__ dpred) {
    __shared__ float red[2 * (kOrdBlock / LTR_WAVE)];
    if (ltr_block_id() * kOrdBlock >= n_docs) return;             // (whole block: the y-padding of a two-dimensional grid)
    const int64_t doc = ltr_block_id() * kOrdBlock + threadIdx.x;
    float ls = 0.f, nv = 0.f;
    if (doc < n_docs) {
        const float y = y_true[doc];
        bool any = false;
        for (int k = 1; k <= n; ++k) {
            // with_ordinals uses the DEFAULT indicator -1 (ordinal.py:39), the mask uses `pad` (:41)
            const float t = (y == -1.f) ? -1.f : (y >= (float)k ? 1.f : 0.f);
            const bool masked = (t == pad);
            const float p = y_pred[doc * n + (k - 1)];
            float l = 0.f, gq = 0.f;
            if (!masked) {
                const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(logf(1.f - p), -100.f);
                l = -(t * lp + (1.f - t) * l1p);
                gq = (p - t) / fmaxf((1.f - p) * p, 1e-12f);
                any = true;
            }
            ls += l;
            if (dpred) dpred[doc * n + (k - 1)] = gq;
        }
        nv = any ? 1.f : 0.f;
    }
    ls = wave_allsum(ls);
    nv = wave_allsum(nv);
    const int w = threadIdx.x / LTR_WAVE;
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0) {
        red[2 * w] = ls;
        red[2 * w + 1] = nv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        for (int i = 0; i < kOrdBlock / LTR_WAVE; ++i) {
            a += red[2 * i];
            b += red[2 * i + 1];
        }
        block_partials[2 * ltr_block_id()] = a;
        block_partials[2 * ltr_block_id() + 1] = b;
    }
}

// Fixed-order two-column sum of the block partials: one workgroup, strided then tree.
__global__ void __launch_bounds__(1024)
reduce_pairs_kernel(const float *__restrict__ in, int64_t n, float *__restrict__ out) {
    __shared__ float red[2 * 16];
    float a = 0.f, b = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        a += in[2 * i];
        b += in[2 * i + 1];
    }
    a = wave_allsum(a);
    b = wave_allsum(b);
    const int w = threadIdx.x / LTR_WAVE;
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0) {
        red[2 * w] = a;
        red[2 * w + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float x = 0.f, y = 0.f;
        for (int i = 0; i < 16; ++i) {
            x += red[2 * i];
            y += red[2 * i + 1];
        }
        out[0] = x;
        out[1] = y;
    }
}

__global__ void __launch_bounds__(1024)
reduce_sum_kernel(const float *__restrict__ in, int64_t n, float scale, float *__restrict__ out) {
    __shared__ float red[16];
    float a = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) a += in[i];
    a = wave_allsum(a);
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0) red[threadIdx.x / LTR_WAVE] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        float x = 0.f;
        for (int i = 0; i < 16; ++i) x += red[i];
        out[0] = x * scale;
    }
}

// ------------------------------------------------------------------------------------------------ ragged batches
// Query q owns document rows offsets[q] .. offsets[q + 1] - 1; a launch handles the queries of an index list (NULL: 0 .. n - 1) that
// share ONE length tier: next_pow2(length) == next_pow2(s_max).  pick_group, make_group's row lanes / column groups and every loop
// with a barrier inside the slate functions depend on the length only through that power of two, so slates of unequal length that
// share a 256-thread workgroup (lengths <= 64) reach every barrier the same number of times, and a launch of equal lengths runs the
// rectangular kernels' geometry exactly (same bits).  LDS is carved at the tier's s_max; each slate stages, zero-fills and pads up
// to its OWN aligned length inside its slice.  A listed query whose length does not belong to the tier (the host layer never
// lists one) gets a NaN loss and no gradient rows: nothing is read or written outside its slice.
struct RaggedSlot {
    long long q;     // query id (index into offsets / slate_loss)
    size_t off;      // first document row
    int S;           // documents; s_max for an idle slot
    bool active;     // a listed query of this tier
    bool misfit;     // a listed query whose length is outside the tier
};

// A slate group is a whole number of waves, so everything about its query is wave-uniform: taking the slot through
// v_readfirstlane keeps the query id, the offset and above all the length S -- and with it the whole group geometry -- in scalar
// registers, as the rectangular kernels have S in a kernel argument.
__device__ __forceinline__ long long wave_uniform(long long v) { return ltr_wave_uniform(v); }

__device__ __forceinline__ RaggedSlot ragged_slot(const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries,
                                                  long long slot, int n_queries, int s_max) {
    slot = wave_uniform(slot);
    RaggedSlot r;
    r.q = 0;
    r.off = 0;
    r.S = s_max;
    r.active = false;
    r.misfit = false;
    if (slot < n_queries) {
        r.q = queries ? (long long)queries[slot] : slot;
        const int64_t a = offsets[r.q], len = offsets[r.q + 1] - a;
        if (len >= 1 && len <= s_max && next_pow2((int)len) == next_pow2(s_max)) {
            r.off = (size_t)a;
            r.S = (int)len;
            r.active = true;
        } else {
            r.misfit = true;
        }
    }
    return r;
}

__global__ void __launch_bounds__(1024)
approxndcg_ragged_kernel(const float *__restrict__ scores, const float *__restrict__ labels, const int64_t *__restrict__ offsets,
                         const int32_t *__restrict__ queries, int n_queries, int s_max, int group, float alpha, float eps,
                         float pad, float gscale, float *__restrict__ slate_loss, float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_cap = (s_max + 3) & ~3;
    const int gid = threadIdx.x / group;
    const RaggedSlot rq = ragged_slot(offsets, queries, ltr_block_id() * (blockDim.x / group) + gid, n_queries, s_max);
    const int S = rq.S;
    const bool active = rq.active;
    float *base = smem + (size_t)gid * (kApproxArrays * s_cap + group + 32);
    float *sc = base, *yl = sc + s_cap, *gn = yl + s_cap, *gg = gn + s_cap, *uu = gg + s_cap, *mk = uu + s_cap;
    ApproxScratch xs;
    xs.um = mk + s_cap;
    const SlateGroup g = make_group(S, group, xs.um + s_cap);
    const size_t off = rq.off;
    approx_ndcg_init(g);
    for (int j = g.t; j < S; j += group) {
        const float y = active ? labels[off + j] : pad;
        sc[j] = active ? scores[off + j] : 0.f;
        stage_label(y, pad, yl[j], gn[j]);
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    const float loss = approx_ndcg_slate(g, sc, yl, gn, gg, uu, mk, alpha, eps, gscale, dscores != nullptr,
                                         [&](int i, float v) { if (active) dst[i] = v; }, NoStamp(), xs);
    if (g.t == 0 && (active || rq.misfit)) slate_loss[rq.q] = active ? loss : NAN;
}

__global__ void __launch_bounds__(1024)
listnet_ragged_kernel(const float *__restrict__ y_true, const float *__restrict__ y_pred, const int64_t *__restrict__ offsets,
                      const int32_t *__restrict__ queries, int n_queries, int s_max, int group, int apply_sigmoid, float gscale,
                      float *__restrict__ slate_loss, float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_cap = (s_max + 3) & ~3;
    const int gid = threadIdx.x / group;
    const RaggedSlot rq = ragged_slot(offsets, queries, ltr_block_id() * (blockDim.x / group) + gid, n_queries, s_max);
    const int S = rq.S;
    const bool active = rq.active;
    float *base = smem + (size_t)gid * (2 * s_cap + group + 32);
    float *yt = base, *yp = yt + s_cap;
    const SlateGroup g = make_group(S, group, yp + s_cap);
    const size_t off = rq.off;
    for (int j = g.t; j < S; j += group) {
        yt[j] = active ? y_true[off + j] : 0.f;
        yp[j] = active ? y_pred[off + j] : 0.f;
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    const float loss = listnet_slate(g, yt, yp, apply_sigmoid != 0, gscale, dscores != nullptr,
                                     [&](int i, float v) { if (active) dst[i] = v; });
    if (g.t == 0 && (active || rq.misfit)) slate_loss[rq.q] = active ? loss : NAN;
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_ragged_kernel(const float *__restrict__ scores, const float *__restrict__ labels, const int64_t *__restrict__ offsets,
                     const int32_t *__restrict__ queries, int n_queries, int s_max, int group, LambdaParams P, float pad,
                     float gscale, float *__restrict__ slate_loss, float *__restrict__ slate_count,
                     float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_cap = (s_max + 3) & ~3;
    const int gid = threadIdx.x / group;
    const RaggedSlot rq = ragged_slot(offsets, queries, ltr_block_id() * (blockDim.x / group) + gid, n_queries, s_max);
    const int S = rq.S;
    const bool active = rq.active;
    float *base = smem + (size_t)gid * (kLambdaArrays * s_cap + group + 32);
    const LambdaLds L = lambda_carve(base, s_cap);
    const SlateGroup g = make_group(S, group, base + kLambdaArrays * s_cap);
    const size_t off = rq.off;
    for (int j = g.t; j < S; j += group) {
        const float y = active ? labels[off + j] : pad;
        L.sc[j] = active ? scores[off + j] : 0.f;
        stage_label(y, pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    float count;
    const float loss = lambda_slate<SCH>(g, L, P, gscale, dscores != nullptr, &count,
                                         [&](int i, float v) { if (active) dst[i] = v; });
    if (g.t == 0 && (active || rq.misfit)) {
        slate_loss[rq.q] = active ? loss : NAN;
        slate_count[rq.q] = active ? count : 0.f;
    }
}

// The rank-space sweep (lambda_blocked_kernel) on a ragged tier: one slate per workgroup of 64 ceil(s_max / 64) threads; the waves
// past a shorter slate's last rank block idle through lambda_slate_blocked's barriers.
template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_blocked_ragged_kernel(const float *__restrict__ scores, const float *__restrict__ labels,
                             const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, int s_max,
                             LambdaParams P, float pad, float gscale, float *__restrict__ slate_loss,
                             float *__restrict__ slate_count, float *__restrict__ dscores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int s_cap = (s_max + 3) & ~3, s64_cap = (s_max + 63) & ~63;
    const RaggedSlot rq = ragged_slot(offsets, queries, ltr_block_id(), n_queries, s_max);
    if (!rq.active) {                            // (whole block: one slate per workgroup)
        if (rq.misfit && threadIdx.x == 0) {
            slate_loss[rq.q] = NAN;
            slate_count[rq.q] = 0.f;
        }
        return;
    }
    const int S = rq.S;
    const LambdaLds L = lambda_carve(smem, s_cap);
    float *rb = smem + kLambdaArrays * s_cap;
    LambdaRankLds R;
    R.rs = rb;
    R.ry = rb + s64_cap;
    R.rg = rb + 2 * s64_cap;
    R.colacc = rb + 3 * s64_cap;
    R.doc_of = reinterpret_cast<int *>(rb + 4 * s64_cap);
    const SlateGroup g = make_group(S, blockDim.x, rb + 5 * s64_cap);
    const size_t off = rq.off;
    for (int j = g.t; j < S; j += blockDim.x) {
        L.sc[j] = scores[off + j];
        stage_label(labels[off + j], pad, L.yl[j], L.gn[j]);
    }
    __syncthreads();
    float *dst = dscores ? dscores + off : nullptr;
    float count;
    const float loss = lambda_slate_blocked<SCH>(g, L, R, P, gscale, dscores != nullptr, &count,
                                                 [&](int i, float v) { dst[i] = v; });
    if (g.t == 0) {
        slate_loss[rq.q] = loss;
        slate_count[rq.q] = count;
    }
}

// ---- The Lambda-type risk losses on a ragged tier: the three kernels above with the slate taken from the
// tier's query list.  ONE slate owns its workgroup, so an idle or misfit slot leaves as a whole block before the first barrier and
// every barrier inside the slate functions is reached by all threads of the block (section 4.9's rule; no mixed-barrier site here).
// The group size comes from the tier's s_max by the geometry function the rectangular launcher calls -- constant inside a tier, which
// depends on the length through next_pow2 only -- so with all lengths equal these are the rectangular launches' bits.  n_docs = the
// documents of the whole batch: system k's column sums start at colsum[k * n_docs].
template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_colsum_sys_ragged_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true, const float *__restrict__ y_base,
                                const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, int s_max,
                                long long n_docs, int nb, int group, LambdaParams P, float pad, float *__restrict__ colsum) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const long long blk = wave_uniform(ltr_block_id());
    if (blk >= (long long)(nb + 2) * n_queries) return;      // (whole block: the y-padding of a two-dimensional grid)
    const int sys = (int)(blk / n_queries);
    const RaggedSlot rq = ragged_slot(offsets, queries, blk - (long long)sys * n_queries, n_queries, s_max);
    if (!rq.active || rq.off + rq.S > (size_t)n_docs) return;      // (whole block) a query outside the tier: its rows stay untouched
    colsum_sys_slate<SCH>(y_pred, y_true, y_base, sys, rq.off, rq.S, nb, group, P, pad, colsum + (size_t)sys * n_docs + rq.off, smem);
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_risk_model_ragged_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true, const float *__restrict__ cache,
                                int cache_stride, const float *__restrict__ ideal_colsum, int n_cached,
                                const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, int s_max,
                                long long n_docs, int group, LambdaParams P, float pad, int lt, float *__restrict__ mat,
                                float *__restrict__ jac) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kEffThreads / LTR_WAVE];
    const RaggedSlot rq = ragged_slot(offsets, queries, ltr_block_id(), n_queries, s_max);
    if (!rq.active || rq.off + rq.S > (size_t)n_docs) {      // (whole block)
        if (rq.misfit && threadIdx.x == 0) mat[(size_t)rq.q * (1 + n_cached)] = NAN;
        return;
    }
    // the rectangular kernel's cache row in two places: the entries in the query's row of `cache`, the column sums at the query's
    // document rows of `ideal_colsum`
    risk_model_slate<SCH>(y_pred, y_true, cache + (size_t)rq.q * cache_stride, ideal_colsum + rq.off, n_cached, rq.off, rq.S, group, P,
                          pad, lt, mat + (size_t)rq.q * (1 + n_cached), jac, smem, red);
}

template <int SCH>
__global__ void __launch_bounds__(1024)
lambda_colsum_sys_bwd_ragged_kernel(const float *__restrict__ y_pred, const float *__restrict__ y_true,
                                    const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, int s_max,
                                    long long n_docs, int group, LambdaParams P, float pad, const float *__restrict__ jac,
                                    const float *__restrict__ coef, int coef_stride, float *__restrict__ dy_pred) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RaggedSlot rq = ragged_slot(offsets, queries, ltr_block_id(), n_queries, s_max);
    if (!rq.active || rq.off + rq.S > (size_t)n_docs) return;      // (whole block) a query outside the tier: its rows stay untouched
    colsum_sys_bwd_slate<SCH>(y_pred, y_true, rq.off, rq.S, group, P, pad, jac, coef[rq.q * coef_stride], dy_pred, smem);
}

// ------------------------------------------------------------------------------------------------ the launch layer
inline int check_slates(const void *a, const void *b, const void *c, int B, int S) {
    if (!a || !b || !c) return LTR_ERR_NULL;
    if (B < 0 || S < 1 || S > LTR_MAX_SLATE) return LTR_ERR_SHAPE;
    return LTR_OK;
}

inline int check_ragged(const void *a, const void *b, const void *c, const void *offsets, int n_queries, int s_max) {
    if (!a || !b || !c || !offsets) return LTR_ERR_NULL;
    if (n_queries < 0 || s_max < 1 || s_max > LTR_MAX_SLATE) return LTR_ERR_SHAPE;
    return LTR_OK;
}

inline int make_lambda_params(int scheme, int k, float sigma, float mu, float eps, int log_base, LambdaParams *P) {
    if (scheme < 0 || scheme > 7) return LTR_ERR_PARAM;
    if (log_base != LTR_LOG_BINARY && log_base != LTR_LOG_NATURAL) return LTR_ERR_PARAM;
    if (!(eps > 0.f)) return LTR_ERR_PARAM;
    P->scheme = scheme;
    P->k = k;
    P->sigma = sigma;
    P->mu = mu;
    P->eps = eps;
    P->log_scale = log_base == LTR_LOG_BINARY ? (float)(1.0 / 0.693147180559945309417) : 1.f;
    P->log_floor = log_base == LTR_LOG_BINARY ? log2f(eps) : logf(eps);
    return LTR_OK;
}

// Geometry.  One function per kernel family, of the slate length alone: a rectangular launcher passes S, a ragged one its tier's
// s_max, and nothing else computes a group size, a block or an LDS size -- which is what makes a ragged launch of equal lengths the
// rectangular launch (the tier rule).

// Slates that share a workgroup of at least 256 threads: `group` threads and `arrays` [S] float arrays in LDS per slate.
struct SlateLaunch {
    int group, block, gpb;
    size_t lds;
    int grid(int n_slates) const { return (n_slates + gpb - 1) / gpb; }
};

inline SlateLaunch shared_plan(int group, int S, int arrays) {
    SlateLaunch L;
    L.group = group;
    L.block = group < 256 ? 256 : group;
    L.gpb = L.block / group;
    L.lds = (size_t)L.gpb * (arrays * ((S + 3) & ~3) + group + 32) * sizeof(float);
    return L;
}

// One thread per document: ListNet's O(S) work per slate, and the column-sum forward kernels (a thread owns a column).
inline int doc_group(int S) { return next_pow2(S) < 64 ? 64 : (next_pow2(S) > 1024 ? 1024 : next_pow2(S)); }

// The document-order pair kernels (approxNDCG, lambda_kernel): pick_group's two threads per row.
inline SlateLaunch plan(int S, int arrays) { return shared_plan(pick_group(S), S, arrays); }
inline SlateLaunch listnet_plan(int S) { return shared_plan(doc_group(S), S, 2); }

// Threads per slate of the one-slate-per-workgroup pair kernels: at least 256, but never more than one wave of column groups
// per row -- row_reduce combines the CG replicas of a row inside ONE wave (CG <= 64), and 256 threads on S <= 2 documents
// would make CG 128 / 256 (doubled rank counts at S = 2).  64 threads at S = 1, 128 at S = 2, unchanged from S = 3 on.
inline int pair_group(int S) {
    int g = pick_group(S) < 256 ? 256 : pick_group(S);
    const int np2 = next_pow2(S);
    while (g / (np2 < g ? np2 : g) > LTR_WAVE) g >>= 1;
    return g;
}

// LDS of a one-slate-per-workgroup Lambda kernel: lambda_carve's arrays, `extra` more [S] arrays, make_group's scratch.
inline size_t pair_lds(int extra, int S, int group) {
    return (size_t)((kLambdaArrays + extra) * ((S + 3) & ~3) + group + 32) * sizeof(float);
}

// lambdaLoss: the rank-space sweep (lambda_blocked_kernel) for 256 <= S <= 1024 and every scheme but ndcgLoss1 -- one slate per
// workgroup, one wave per 64 ranks, LambdaRankLds next to lambda_carve's arrays -- and lambda_kernel on plan() everywhere else.
struct LambdaLaunch : SlateLaunch {
    bool blocked;
};

inline LambdaLaunch lambda_plan(int S, int scheme) {
    LambdaLaunch L;
    L.blocked = S >= 256 && S <= 1024 && scheme != LTR_SCHEME_NDCG_LOSS1;
    if (!L.blocked) {
        static_cast<SlateLaunch &>(L) = plan(S, kLambdaArrays);
        return L;
    }
    const int s64 = (S + 63) & ~63;
    L.group = L.block = s64;
    L.gpb = 1;
    L.lds = (size_t)(kLambdaArrays * ((S + 3) & ~3) + 5 * s64 + s64 + 32) * sizeof(float);
    return L;
}

// Every launch of this file: the LDS opt-in above 64 KB, `blocks` workgroups through ltr_grid, the launch's status.
template <class... KA, class... A>
inline int launch(void (*kernel)(KA...), long long blocks, int block, size_t lds, void *stream, A... args) {
    if (int rc = allow_lds(kernel, lds)) return rc;
    hipLaunchKernelGGL(kernel, ltr_grid(blocks), dim3(block), lds, (hipStream_t)stream, static_cast<KA>(args)...);
    return launch_status();
}

// The Lambda kernels are templates on the weighting scheme: f(std::integral_constant<int, SCH>()) for a scheme that
// make_lambda_params has accepted (0 .. 7).
template <class F>
inline int with_scheme(int scheme, F f) {
    switch (scheme) {
        case 0: return f(std::integral_constant<int, 0>());
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
        default: return f(std::integral_constant<int, 7>());
    }
}

}  // namespace

extern "C" {

int ltr_abi_version(void) { return LTR_ABI_VERSION; }

const char *ltr_error_string(int code) {
    switch (code) {
        case LTR_OK: return "ok";
        case LTR_ERR_NULL: return "ltr: required pointer is NULL";
        case LTR_ERR_SHAPE: return "ltr: shape outside supported range";
        case LTR_ERR_PARAM: return "ltr: invalid parameter";
        case LTR_ERR_ALIGN: return "ltr: pointer not aligned as required";
        case LTR_ERR_IO: return "ltr: cannot open / map the input file";
        case LTR_ERR_PARSE: return "ltr: malformed input line";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "ltr: unknown error";
    }
}

int ltr_reduce_sum_f32(const float *in, int64_t n, float scale, float *out, void *stream) {
    if (!in || !out) return LTR_ERR_NULL;
    if (n < 0) return LTR_ERR_SHAPE;
    return launch(reduce_sum_kernel, 1, 1024, 0, stream, in, n, scale, out);
}

int ltr_approxndcg_fwd_bwd(const float *scores, const float *labels, int B, int S, float alpha, float eps,
                           float pad, float grad_scale, float *slate_loss, float *dscores, void *stream) {
    if (int rc = check_slates(scores, labels, slate_loss, B, S)) return rc;
    if (B == 0) return LTR_OK;
    const SlateLaunch L = plan(S, kApproxArrays);
    return launch(approxndcg_kernel, L.grid(B), L.block, L.lds, stream, scores, labels, B, S, L.group, alpha, eps, pad, grad_scale,
                  slate_loss, dscores);
}

int ltr_listnet_fwd_bwd(const float *y_true, const float *y_pred, int B, int S, int apply_sigmoid,
                        float grad_scale, float *slate_loss, float *dscores, void *stream) {
    if (int rc = check_slates(y_true, y_pred, slate_loss, B, S)) return rc;
    if (B == 0) return LTR_OK;
    const SlateLaunch L = listnet_plan(S);
    return launch(listnet_kernel, L.grid(B), L.block, L.lds, stream, y_true, y_pred, B, S, L.group, apply_sigmoid, grad_scale,
                  slate_loss, dscores);
}

int ltr_lambda_fwd_bwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                       float mu, float eps, float pad, int log_base, float grad_scale, float *slate_loss,
                       float *slate_count, float *dscores, void *stream) {
    if (int rc = check_slates(scores, labels, slate_loss, B, S)) return rc;
    if (!slate_count) return LTR_ERR_NULL;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const LambdaLaunch L = lambda_plan(S, scheme);
    return with_scheme(scheme, [&](auto sch) {
        constexpr int SCH = decltype(sch)::value;
        if constexpr (SCH != LTR_SCHEME_NDCG_LOSS1)      // the rank-space sweep is not built for ndcgLoss1: lambda_plan never picks it
            if (L.blocked)
                return launch(lambda_blocked_kernel<SCH>, L.grid(B), L.block, L.lds, stream, scores, labels, B, S, P, pad, grad_scale,
                              slate_loss, slate_count, dscores);
        return launch(lambda_kernel<SCH>, L.grid(B), L.block, L.lds, stream, scores, labels, B, S, L.group, P, pad, grad_scale,
                      slate_loss, slate_count, dscores);
    });
}

int ltr_lambda_pairs_fwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                         float mu, float eps, float pad, int log_base, float *losses, uint8_t *keep,
                         int32_t *rank, void *stream) {
    if (int rc = check_slates(scores, labels, losses, B, S)) return rc;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = pair_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_pairs_fwd_kernel<decltype(sch)::value>, B, group, pair_lds(1, S, group), stream, scores, labels, B, S,
                      group, P, pad, losses, keep, rank);
    });
}

int ltr_lambda_pairs_bwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                         float mu, float eps, float pad, int log_base, const float *grad_losses,
                         float *dscores, void *stream) {
    if (int rc = check_slates(scores, labels, dscores, B, S)) return rc;
    if (!grad_losses) return LTR_ERR_NULL;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = pair_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_pairs_bwd_kernel<decltype(sch)::value>, B, group, pair_lds(0, S, group), stream, scores, labels, B, S,
                      group, P, pad, grad_losses, 0, dscores);
    });
}

int ltr_lambda_colsum_fwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                          float mu, float eps, float pad, int log_base, float *colsum, void *stream) {
    if (int rc = check_slates(scores, labels, colsum, B, S)) return rc;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = doc_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_colsum_fwd_kernel<decltype(sch)::value>, B, group, pair_lds(1, S, group), stream, scores, labels, B, S,
                      group, P, pad, colsum);
    });
}

int ltr_lambda_colsum_bwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                          float mu, float eps, float pad, int log_base, const float *grad_colsum, float *dscores,
                          void *stream) {
    if (int rc = check_slates(scores, labels, dscores, B, S)) return rc;
    if (!grad_colsum) return LTR_ERR_NULL;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = pair_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_pairs_bwd_kernel<decltype(sch)::value>, B, group, pair_lds(0, S, group), stream, scores, labels, B, S,
                      group, P, pad, grad_colsum, 1, dscores);
    });
}

int ltr_lambda_colsum_sys_fwd(const float *y_pred, const float *y_true, const float *y_base, int B, int S, int n_base, int scheme,
                              int k, float sigma, float mu, float eps, float pad, int log_base, float *colsum, void *stream) {
    if (int rc = check_slates(y_pred, y_true, colsum, B, S)) return rc;
    if (n_base < 0 || n_base > 4096 || (n_base > 0 && !y_base)) return n_base > 0 && !y_base ? LTR_ERR_NULL : LTR_ERR_SHAPE;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = doc_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_colsum_sys_fwd_kernel<decltype(sch)::value>, (long long)(n_base + 2) * B, group, pair_lds(1, S, group),
                      stream, y_pred, y_true, y_base, B, S, n_base, group, P, pad, colsum);
    });
}

int ltr_lambda_colsum_sys_bwd(const float *y_pred, const float *y_true, int B, int S, int scheme, int k, float sigma, float mu,
                              float eps, float pad, int log_base, const float *grad_colsum, float *dy_pred, void *stream) {
    if (int rc = check_slates(y_pred, y_true, dy_pred, B, S)) return rc;
    if (!grad_colsum) return LTR_ERR_NULL;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = pair_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_colsum_sys_bwd_kernel<decltype(sch)::value>, B, group, pair_lds(1, S, group), stream, y_pred, y_true, B,
                      S, group, P, pad, grad_colsum, nullptr, 0, dy_pred);
    });
}

int ltr_lambda_risk_model_fwd(const float *y_pred, const float *y_true, const float *cache, int cache_stride, int n_cached, int B, int S,
                              int scheme, int k, float sigma, float mu, float eps, float pad, int log_base, int lt, float *mat, float *jac,
                              void *stream) {
    if (int rc = check_slates(y_pred, y_true, mat, B, S)) return rc;
    if (!cache || !jac) return LTR_ERR_NULL;
    if (S < 2 || S > 2048 || n_cached < 0 || n_cached > 65 || cache_stride < n_cached + S) return LTR_ERR_SHAPE;
    if (lt < 1 || lt > 3) return LTR_ERR_PARAM;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = doc_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_risk_model_fwd_kernel<decltype(sch)::value>, B, group, pair_lds(2, S, group), stream, y_pred, y_true,
                      cache, cache_stride, n_cached, B, S, group, P, pad, lt, mat, jac);
    });
}

int ltr_lambda_colsum_sys_bwd_coef(const float *y_pred, const float *y_true, int B, int S, int scheme, int k, float sigma, float mu,
                                   float eps, float pad, int log_base, const float *jac, const float *coef, int coef_stride, float *dy_pred,
                                   void *stream) {
    if (int rc = check_slates(y_pred, y_true, dy_pred, B, S)) return rc;
    if (!jac || !coef) return LTR_ERR_NULL;
    if (coef_stride < 1) return LTR_ERR_SHAPE;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (B == 0) return LTR_OK;
    const int group = pair_group(S);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_colsum_sys_bwd_kernel<decltype(sch)::value>, B, group, pair_lds(1, S, group), stream, y_pred, y_true, B,
                      S, group, P, pad, jac, coef, coef_stride, dy_pred);
    });
}

int ltr_approxndcg_ragged_fwd_bwd(const float *scores, const float *labels, const int64_t *offsets, const int32_t *queries,
                                  int n_queries, int s_max, float alpha, float eps, float pad, float grad_scale, float *slate_loss,
                                  float *dscores, void *stream) {
    if (int rc = check_ragged(scores, labels, slate_loss, offsets, n_queries, s_max)) return rc;
    if (n_queries == 0) return LTR_OK;
    const SlateLaunch L = plan(s_max, kApproxArrays);
    return launch(approxndcg_ragged_kernel, L.grid(n_queries), L.block, L.lds, stream, scores, labels, offsets, queries, n_queries,
                  s_max, L.group, alpha, eps, pad, grad_scale, slate_loss, dscores);
}

int ltr_listnet_ragged_fwd_bwd(const float *y_true, const float *y_pred, const int64_t *offsets, const int32_t *queries,
                               int n_queries, int s_max, int apply_sigmoid, float grad_scale, float *slate_loss, float *dscores,
                               void *stream) {
    if (int rc = check_ragged(y_true, y_pred, slate_loss, offsets, n_queries, s_max)) return rc;
    if (n_queries == 0) return LTR_OK;
    const SlateLaunch L = listnet_plan(s_max);
    return launch(listnet_ragged_kernel, L.grid(n_queries), L.block, L.lds, stream, y_true, y_pred, offsets, queries, n_queries,
                  s_max, L.group, apply_sigmoid, grad_scale, slate_loss, dscores);
}

int ltr_lambda_ragged_fwd_bwd(const float *scores, const float *labels, const int64_t *offsets, const int32_t *queries,
                              int n_queries, int s_max, int scheme, int k, float sigma, float mu, float eps, float pad,
                              int log_base, float grad_scale, float *slate_loss, float *slate_count, float *dscores,
                              void *stream) {
    if (int rc = check_ragged(scores, labels, slate_loss, offsets, n_queries, s_max)) return rc;
    if (!slate_count) return LTR_ERR_NULL;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (n_queries == 0) return LTR_OK;
    const LambdaLaunch L = lambda_plan(s_max, scheme);
    return with_scheme(scheme, [&](auto sch) {
        constexpr int SCH = decltype(sch)::value;
        if constexpr (SCH != LTR_SCHEME_NDCG_LOSS1)
            if (L.blocked)
                return launch(lambda_blocked_ragged_kernel<SCH>, L.grid(n_queries), L.block, L.lds, stream, scores, labels, offsets,
                              queries, n_queries, s_max, P, pad, grad_scale, slate_loss, slate_count, dscores);
        return launch(lambda_ragged_kernel<SCH>, L.grid(n_queries), L.block, L.lds, stream, scores, labels, offsets, queries,
                      n_queries, s_max, L.group, P, pad, grad_scale, slate_loss, slate_count, dscores);
    });
}

int ltr_lambda_colsum_sys_ragged_fwd(const float *y_pred, const float *y_true, const float *y_base, const int64_t *offsets,
                                     const int32_t *queries, int n_queries, int s_max, int64_t n_docs, int n_base, int scheme, int k,
                                     float sigma, float mu, float eps, float pad, int log_base, float *colsum, void *stream) {
    if (int rc = check_ragged(y_pred, y_true, colsum, offsets, n_queries, s_max)) return rc;
    if (n_base > 0 && !y_base) return LTR_ERR_NULL;
    if (n_base < 0 || n_base > 4096 || n_docs < 0) return LTR_ERR_SHAPE;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (n_queries == 0) return LTR_OK;
    const int group = doc_group(s_max);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_colsum_sys_ragged_kernel<decltype(sch)::value>, (long long)(n_base + 2) * n_queries, group,
                      pair_lds(1, s_max, group), stream, y_pred, y_true, y_base, offsets, queries, n_queries, s_max, n_docs, n_base,
                      group, P, pad, colsum);
    });
}

int ltr_lambda_risk_model_ragged_fwd(const float *y_pred, const float *y_true, const float *cache, int cache_stride,
                                     const float *ideal_colsum, int n_cached, const int64_t *offsets, const int32_t *queries,
                                     int n_queries, int s_max, int64_t n_docs, int scheme, int k, float sigma, float mu, float eps,
                                     float pad, int log_base, int lt, float *mat, float *jac, void *stream) {
    if (int rc = check_ragged(y_pred, y_true, mat, offsets, n_queries, s_max)) return rc;
    if (!ideal_colsum || !jac || (n_cached > 0 && !cache)) return LTR_ERR_NULL;
    if (s_max < 2 || n_cached < 0 || n_cached > 65 || cache_stride < n_cached || n_docs < 0) return LTR_ERR_SHAPE;
    if (lt < 1 || lt > 3) return LTR_ERR_PARAM;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (n_queries == 0) return LTR_OK;
    const int group = doc_group(s_max);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_risk_model_ragged_kernel<decltype(sch)::value>, n_queries, group, pair_lds(2, s_max, group), stream,
                      y_pred, y_true, cache, cache_stride, ideal_colsum, n_cached, offsets, queries, n_queries, s_max, n_docs, group, P,
                      pad, lt, mat, jac);
    });
}

int ltr_lambda_colsum_sys_ragged_bwd_coef(const float *y_pred, const float *y_true, const int64_t *offsets, const int32_t *queries,
                                          int n_queries, int s_max, int64_t n_docs, int scheme, int k, float sigma, float mu, float eps,
                                          float pad, int log_base, const float *jac, const float *coef, int coef_stride, float *dy_pred,
                                          void *stream) {
    if (int rc = check_ragged(y_pred, y_true, dy_pred, offsets, n_queries, s_max)) return rc;
    if (!jac || !coef) return LTR_ERR_NULL;
    if (coef_stride < 1 || n_docs < 0) return LTR_ERR_SHAPE;
    LambdaParams P;
    if (int rc = make_lambda_params(scheme, k, sigma, mu, eps, log_base, &P)) return rc;
    if (n_queries == 0) return LTR_OK;
    const int group = pair_group(s_max);
    return with_scheme(scheme, [&](auto sch) {
        return launch(lambda_colsum_sys_bwd_ragged_kernel<decltype(sch)::value>, n_queries, group, pair_lds(1, s_max, group), stream,
                      y_pred, y_true, offsets, queries, n_queries, s_max, n_docs, group, P, pad, jac, coef, coef_stride, dy_pred);
    });
}

int64_t ltr_ordinal_num_blocks(int64_t n_docs) { return n_docs <= 0 ? 0 : (n_docs + kOrdBlock - 1) / kOrdBlock; }

int ltr_ordinal_fwd_bwd(const float *y_pred, const float *y_true, int64_t n_docs, int n, float pad,
                        float *block_partials, float *sums, float *dpred, void *stream) {
    if (!y_pred || !y_true || !block_partials || !sums) return LTR_ERR_NULL;
    if (n_docs < 0 || n < 1 || n > 64 || ltr_ordinal_num_blocks(n_docs) > 0x7fffffff) return LTR_ERR_SHAPE;
    const int64_t nb = ltr_ordinal_num_blocks(n_docs);
    if (nb > 0)
        if (int rc = launch(ordinal_kernel, nb, kOrdBlock, 0, stream, y_pred, y_true, n_docs, n, pad, block_partials, dpred)) return rc;
    return launch(reduce_pairs_kernel, 1, 1024, 0, stream, block_partials, nb, sums);
}

}  // extern "C"
