// ltr_linear.hip -- the FC-only make_model ranker (multiLayer.py:13-51, :94-124, :127-149) as ONE scoring vector (gfx950).
//
// FCModel and OutputLayer hard-wire nn.Identity activations (multiLayer.py:29, :105).  With no active dropout the network
//     h_0 = x  (or  gamma o xhat + beta  with input_norm: nn.LayerNorm, eps 1e-5, biased variance)
//     h_i = W_i h_{i-1} + b_i          i = 1..L
//     s   = w_o h_L + b_o
// is the affine map  s = w_eff . h_0 + b_eff  with
//     v_L = w_o,   v_{i-1} = v_i W_i,   w_eff = v_0 in R^F,   b_eff = b_o + sum_i v_i . b_i.
// With input_norm the kernels score  (w_eff o gamma) . xhat + (w_eff . beta + b_eff).
//
// Gradient.  With ds_d = d loss / d s_d, the only quantities the documents contribute are
//     G_1 = sum_d ds_d        and    Ghat = sum_d ds_d h_0,d   (sum_d ds_d xhat_d with input_norm).
// The chain rule of the layer-by-layer network then reads, per step:
//     H_0 = Ghat  (gamma o Ghat + beta G_1 with input_norm)          = sum_d ds_d h_0,d
//     H_i = W_i H_{i-1} + b_i G_1                                    = sum_d ds_d h_i,d
//     dW_i = v_i^T H_{i-1}^T,   db_i = v_i^T G_1,   dw_o = H_L^T,   db_o = G_1
//     input_norm:  dgamma = w_eff o Ghat,   dbeta = w_eff G_1
// -- exactly the reference autograd's sums (d loss / d h_i,d = ds_d v_i), taken in another order.
//
// Launch plan of one training step (ltr_mi355x/linear.py):
//     ltr_linear_fold          1 workgroup   v_i chain and w_eff / b_eff in fp64                  (every step, live parameters)
//     ltr_linear_fused_step    S in {32, 64, 128}, F <= 256, F % 4 == 0: scores + listwise loss + Ghat partials in ONE launch
//       or ltr_linear_scores -> ltr_*_fwd_bwd (the standalone loss kernels) -> ltr_linear_grad_partials   (any 1 <= S <= 2048)
//     ltr_linear_unfold_grads  fixed-order reduction of the partials, H_i chain in fp64, every gradient into the flat buffer
// Scoring and gradient are both ONE-column contractions (X w and X^T ds): no matrix pipe to feed, no MFMA -- plain fp32 VALU
// dot products with 16-lane DPP row sums, bound by the HBM read of X.  No float atomics anywhere: every sum has a fixed order.
#include "../../include/ltr_mi355x.h"
#include "ltr_slate_losses.h"

using namespace ltr;

namespace {

constexpr int kLinMaxLayers = LTR_LINEAR_MAX_LAYERS;
constexpr int kLinMaxF = 1024;          // multi-launch path (grad partials keep F / 64 accumulators per lane)
constexpr int kLinFusedMaxF = 256;      // one-launch path (the 128-document X tile lives in LDS)
constexpr int kTile = 128;              // documents per super-tile of the one-launch kernel
constexpr float kLnEps = 1e-5f;         // nn.LayerNorm default (multiLayer.py:28)

// The network by value: widths, parameter pointers (LTRModel._ltr_params() order), flat-gradient and workspace offsets.
struct LinNet {
    int L, F, ln;
    int n[kLinMaxLayers + 1];                      // n[0] = F, n[i] = out_features of layer i
    const float *W[kLinMaxLayers], *b[kLinMaxLayers];
    const float *wo, *bo, *gamma, *beta;
    long long fW[kLinMaxLayers], fb[kLinMaxLayers], fwo, fbo, fgamma, fbeta;   // offsets into the flat gradient
    int vo[kLinMaxLayers + 1], ho[kLinMaxLayers + 1], go;                       // offsets into ws (doubles): v_i, H_i, [Ghat | G_1]
    long long nW;                                                               // sum_i n_i n_{i-1}
};

// params: host array of device pointers [gamma, beta]? + [W_1, b_1, ..., W_L, b_L] + [w_o, b_o]
int make_net(int n_layers, int F, const int *sizes, int input_norm, const float *const *params, LinNet &N) {
    if (!params || (n_layers > 0 && !sizes)) return LTR_ERR_NULL;
    if (n_layers < 0 || n_layers > kLinMaxLayers || F < 1 || F > 65536) return LTR_ERR_SHAPE;
    if (input_norm != 0 && input_norm != 1) return LTR_ERR_PARAM;
    N.L = n_layers;
    N.F = F;
    N.ln = input_norm;
    N.n[0] = F;
    int p = 0;
    long long off = 0;
    N.gamma = N.beta = nullptr;
    N.fgamma = N.fbeta = -1;
    if (input_norm) {
        N.gamma = params[p++];
        N.beta = params[p++];
        N.fgamma = off;
        N.fbeta = off + F;
        off += 2 * (long long)F;
        if (!N.gamma || !N.beta) return LTR_ERR_NULL;
    }
    N.nW = 0;
    for (int i = 1; i <= n_layers; ++i) {
        const int w = sizes[i - 1];
        if (w < 1 || w > 65536) return LTR_ERR_SHAPE;
        N.n[i] = w;
        N.W[i - 1] = params[p++];
        N.b[i - 1] = params[p++];
        if (!N.W[i - 1] || !N.b[i - 1]) return LTR_ERR_NULL;
        N.fW[i - 1] = off;
        off += (long long)w * N.n[i - 1];
        N.fb[i - 1] = off;
        off += w;
        N.nW += (long long)w * N.n[i - 1];
    }
    N.wo = params[p++];
    N.bo = params[p++];
    if (!N.wo || !N.bo) return LTR_ERR_NULL;
    N.fwo = off;
    N.fbo = off + N.n[n_layers];
    int o = 0;
    for (int i = 0; i <= n_layers; ++i) { N.vo[i] = o; o += N.n[i]; }
    for (int i = 0; i <= n_layers; ++i) { N.ho[i] = o; o += N.n[i]; }
    N.go = o;
    return LTR_OK;
}

// Sum of v over the block in a fixed tree order (every thread gets the same bits).  All threads must call it.
__device__ double block_sum_f64(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- fold
// One workgroup of 1024 threads.  ws (fp64): v_0 .. v_L.  weff [F + 2]: w_eff (o gamma), the constant term, sum of the first F.
__global__ void __launch_bounds__(1024) linear_fold_kernel(LinNet N, double *__restrict__ ws, float *__restrict__ weff) {
    __shared__ double red[1024];
    const int t = threadIdx.x, nt = blockDim.x;
    double *vL = ws + N.vo[N.L];
    for (int j = t; j < N.n[N.L]; j += nt) vL[j] = (double)N.wo[j];
    __syncthreads();
    for (int i = N.L; i >= 1; --i) {                 // v_{i-1}[k] = sum_j v_i[j] W_i[j][k]: thread per k, rows read coalesced
        const double *vi = ws + N.vo[i];
        double *vp = ws + N.vo[i - 1];
        const float *W = N.W[i - 1];
        const int nin = N.n[i - 1], nout = N.n[i];
        for (int k = t; k < nin; k += nt) {
            double a = 0.0;
            for (int j = 0; j < nout; ++j) a += vi[j] * (double)W[(size_t)j * nin + k];
            vp[k] = a;
        }
        __syncthreads();
    }
    double c = 0.0;                                   // sum_i v_i . b_i  (+ w_eff . beta)
    for (int i = 1; i <= N.L; ++i) {
        const double *vi = ws + N.vo[i];
        for (int j = t; j < N.n[i]; j += nt) c += vi[j] * (double)N.b[i - 1][j];
    }
    double sw = 0.0;
    const double *v0 = ws + N.vo[0];
    for (int f = t; f < N.F; f += nt) {
        double w = v0[f];
        if (N.ln) {
            c += w * (double)N.beta[f];
            w *= (double)N.gamma[f];
        }
        weff[f] = (float)w;
        sw += w;
    }
    c = block_sum_f64(c, red);
    sw = block_sum_f64(sw, red);
    if (t == 0) {
        weff[N.F] = (float)(c + (double)N.bo[0]);
        weff[N.F + 1] = (float)sw;
    }
}

// ---------------------------------------------------------------------------------------------------------- unfold (1)
// Partials [grid][F + 1] -> ws Ghat [F], G_1: blocks of 64 columns x 16 row sets, combined in a fixed order.
__global__ void __launch_bounds__(1024) linear_reduce_partials_kernel(const float *__restrict__ partials, int grid, int F1,
                                                                      double *__restrict__ out) {
    __shared__ double red[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double a = 0.0;
    if (c < F1)
        for (int r = w; r < grid; r += 16) a += (double)partials[(size_t)r * F1 + c];
    red[w][lane] = a;
    __syncthreads();
    if (w == 0 && c < F1) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += red[k][lane];
        out[c] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------- unfold (2)
// One workgroup: H_0 .. H_L in fp64 (one wave per output row, lanes over the row, fixed butterfly), then the vector gradients.
__global__ void __launch_bounds__(1024) linear_unfold_kernel(LinNet N, double *__restrict__ ws, float *__restrict__ flat) {
    const int t = threadIdx.x, nt = blockDim.x;
    const int lane = t & 63, wv = t >> 6, nw = nt >> 6;
    const double *gh = ws + N.go;
    const double g1 = gh[N.F];
    const double *v0 = ws + N.vo[0];
    double *h0 = ws + N.ho[0];
    for (int f = t; f < N.F; f += nt) {
        double h = gh[f];
        if (N.ln) {
            flat[N.fgamma + f] = (float)(v0[f] * gh[f]);
            flat[N.fbeta + f] = (float)(v0[f] * g1);
            h = (double)N.gamma[f] * gh[f] + (double)N.beta[f] * g1;
        }
        h0[f] = h;
    }
    __syncthreads();
    for (int i = 1; i <= N.L; ++i) {
        const double *hp = ws + N.ho[i - 1];
        double *hi = ws + N.ho[i];
        const float *W = N.W[i - 1];
        const int nin = N.n[i - 1], nout = N.n[i];
        for (int j = wv; j < nout; j += nw) {
            double a = 0.0;
            for (int k = lane; k < nin; k += 64) a += (double)W[(size_t)j * nin + k] * hp[k];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) hi[j] = a + (double)N.b[i - 1][j] * g1;
        }
        __syncthreads();
        const double *vi = ws + N.vo[i];
        for (int j = t; j < nout; j += nt) flat[N.fb[i - 1] + j] = (float)(vi[j] * g1);
    }
    const double *hL = ws + N.ho[N.L];
    for (int j = t; j < N.n[N.L]; j += nt) flat[N.fwo + j] = (float)hL[j];
    if (t == 0) flat[N.fbo] = (float)g1;
}

// ---------------------------------------------------------------------------------------------------------- unfold (3)
// dW_i[j][k] = v_i[j] H_{i-1}[k] for every layer: one element per thread.
__global__ void __launch_bounds__(256) linear_outer_kernel(LinNet N, const double *__restrict__ ws, float *__restrict__ flat) {
    long long e = ltr_block_id() * 256 + threadIdx.x;
    if (e >= N.nW) return;
    for (int i = 1; i <= N.L; ++i) {
        const long long sz = (long long)N.n[i] * N.n[i - 1];
        if (e < sz) {
            const int j = (int)(e / N.n[i - 1]), k = (int)(e - (long long)j * N.n[i - 1]);
            flat[N.fW[i - 1] + e] = (float)(ws[N.vo[i] + j] * ws[N.ho[i - 1] + k]);
            return;
        }
        e -= sz;
    }
}

// ------------------------------------------------------------------------------------------------ multi-launch: scores
// One document per 16-lane DPP row (16 documents per 256-thread block); lanes stride the features (float4 when VEC).
// input_norm: fp64 row statistics in the same pass; stats[d] = (mean, rstd).
template <bool VEC, bool LN>
__global__ void __launch_bounds__(256) linear_scores_kernel(const float *__restrict__ X, long long n, int F,
                                                            const float *__restrict__ weff, float *__restrict__ scores,
                                                            float *__restrict__ stats) {
    const long long d = ltr_block_id() * 16 + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const bool live = d < n;
    const float *x = X + (live ? d : 0) * (long long)F;
    float dot = 0.f;
    double sx = 0.0, sxx = 0.0, swx = 0.0;
    if (live) {
        if (VEC) {
            const float4 *x4 = reinterpret_cast<const float4 *>(x);
            const float4 *w4 = reinterpret_cast<const float4 *>(weff);
            for (int c = l; c < (F >> 2); c += 16) {
                const float4 v = x4[c], w = w4[c];
                if (LN) {
                    const double a[4] = {v.x, v.y, v.z, v.w}, b[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        sx += a[q];
                        sxx += a[q] * a[q];
                        swx += a[q] * b[q];
                    }
                } else {
                    dot = fmaf(v.x, w.x, dot);
                    dot = fmaf(v.y, w.y, dot);
                    dot = fmaf(v.z, w.z, dot);
                    dot = fmaf(v.w, w.w, dot);
                }
            }
        } else {
            for (int f = l; f < F; f += 16) {
                const float v = x[f], w = weff[f];
                if (LN) {
                    sx += v;
                    sxx += (double)v * v;
                    swx += (double)v * w;
                } else {
                    dot = fmaf(v, w, dot);
                }
            }
        }
    }
    if (LN) {
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) {
            sx += __shfl_xor(sx, o, 16);
            sxx += __shfl_xor(sxx, o, 16);
            swx += __shfl_xor(swx, o, 16);
        }
        if (live && l == 0) {
            const double mu = sx / F;
            const double var = fmax(sxx / F - mu * mu, 0.0);
            const double rstd = 1.0 / sqrt(var + (double)kLnEps);
            scores[d] = (float)(rstd * (swx - mu * (double)weff[F + 1]) + (double)weff[F]);
            stats[2 * d] = (float)mu;
            stats[2 * d + 1] = (float)rstd;
        }
    } else {
        dot += LTR_DPP(dot, LTR_DPP_XOR1);
        dot += LTR_DPP(dot, LTR_DPP_XOR2);
        dot += LTR_DPP(dot, LTR_DPP_HALF_MIRROR);
        dot += LTR_DPP(dot, LTR_DPP_MIRROR);
        if (live && l == 0) scores[d] = dot + weff[F];
    }
}

// ---------------------------------------------------------------------------------------- multi-launch: gradient partials
// Workgroup g takes a contiguous document range; wave w its documents w, w + 4, ...; lane l features l + 64 k.
// partials[g] = [sum_d ds_d xhat_d (F) | sum_d ds_d].  Fixed order everywhere.
template <bool LN>
__global__ void __launch_bounds__(256) linear_grad_partials_kernel(const float *__restrict__ X, long long n, int F,
                                                                   const float *__restrict__ ds, const float *__restrict__ stats,
                                                                   float *__restrict__ partials) {
    constexpr int KM = kLinMaxF / 64;
    __shared__ float red[4][kLinMaxF + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long d0 = (long long)blockIdx.x * per, d1 = d0 + per < n ? d0 + per : n;
    float acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[k] = 0.f;
    float g1 = 0.f;
    for (long long d = d0 + w; d < d1; d += 4) {
        const float g = ds[d];
        float a = g, m = 0.f;
        if (LN) {
            a = g * stats[2 * d + 1];
            m = stats[2 * d];
        }
        g1 += g;
        const float *x = X + d * (long long)F;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int f = lane + 64 * k;
            if (f < F) acc[k] = fmaf(a, LN ? x[f] - m : x[f], acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        const int f = lane + 64 * k;
        if (f < F) red[w][f] = acc[k];
    }
    if (lane == 0) red[w][kLinMaxF] = g1;
    __syncthreads();
    float *out = partials + (size_t)blockIdx.x * (F + 1);
    for (int f = threadIdx.x; f <= F; f += 256) {
        const int src = f == F ? kLinMaxF : f;
        out[f] = (red[0][src] + red[1][src]) + (red[2][src] + red[3][src]);
    }
}

// ------------------------------------------------------------------------------------------------- one-launch fused step
// Persistent 256-thread workgroups over 128-document super-tiles (128 / S slates of S documents).  Per tile:
//   1. X tile -> LDS once (float4, row stride F + 4), rows past the batch zero;
//   2. scores: 16-lane DPP row sums over the LDS rows (input_norm: mean pass, then variance and the centred dot product);
//   3. the listwise loss on the LDS-resident scores by the device functions of ltr_slate_losses.h, one slate group
//      (pick_group(S) = 2 S threads) per slate, d loss / d s into LDS;
//   4. Ghat += sum_d ds_d xhat_d from the same LDS rows, thread f owning feature f in a register across the tiles.
// Each workgroup writes its partial [Ghat | G_1] once.
struct FusedArgs {
    const float *X, *labels, *weff;
    int B, S, F;
    float alpha, eps, pad, gscale;
    int apply_sigmoid;
    LambdaParams lp;
    float *slate_loss, *slate_count, *partials;
};

constexpr int kLossArrays = 7;   // approxNDCG: sc yl gn gg uu mk um;  lambdaLoss: sc yl gn w1 invd delta rk;  ListNet: 2

inline size_t fused_lds_bytes(int F, int S) {
    const int group = pick_group(S), gpb = 256 / group;
    return ((size_t)kTile * (F + 4) + 4 * kTile + (size_t)gpb * (kLossArrays * S + group + 32)) * sizeof(float);
}

// LK: 0 approxNDCG, 1 ListNet, 2 lambdaLoss (SCH = weighing scheme)
template <int LK, int SCH, bool LN>
__global__ void __launch_bounds__(256) linear_fused_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = a.F, S = a.S, LD = F + 4, F4 = F >> 2;
    float *xs = smem;                          // [128][LD]
    float *sc = xs + kTile * LD;               // [128] scores
    float *dsl = sc + kTile;                   // [128] d loss / d s
    float *mu = dsl + kTile;                   // [128] row mean      (input_norm)
    float *rs = mu + kTile;                    // [128] row 1 / std   (input_norm)
    float *lb = rs + kTile;                    // per slate group: kLossArrays * S + group + 32
    const int group = 2 * S, gpb = 256 / group;   // = pick_group(S) for S in {32, 64, 128}
    const int tid = threadIdx.x;
    const int gid = tid / group;
    float *gb = lb + (size_t)gid * (kLossArrays * S + group + 32);
    const long long n = (long long)a.B * S;
    const long long tiles = (n + kTile - 1) / kTile;
    const int r = tid >> 4, l = tid & 15;      // DPP row r scores documents r, r + 16, ...
    float acc = 0.f, g1 = 0.f;                 // Ghat[tid] (tid < F), G_1
    if (LK == 0) {
        const SlateGroup g0 = make_group(S, group, gb + kLossArrays * S, tid);
        approx_ndcg_init(g0);
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();                       // previous tile's LDS reads done
        const long long base = tile * kTile;
        const int nd = (int)(n - base < kTile ? n - base : kTile);
        const float4 *src = reinterpret_cast<const float4 *>(a.X + base * F);
        for (int q = tid; q < kTile * F4; q += 256) {
            const int d = q / F4, c = q - d * F4;
            const float4 v = d < nd ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(xs + d * LD + 4 * c) = v;
        }
        if (tid < kTile) dsl[tid] = 0.f;
        __syncthreads();
        for (int d = r; d < kTile; d += 16) {
            const float *x = xs + d * LD;
            if (LN) {
                float s1 = 0.f;
                for (int f = l; f < F; f += 16) s1 += x[f];
                s1 += LTR_DPP(s1, LTR_DPP_XOR1);
                s1 += LTR_DPP(s1, LTR_DPP_XOR2);
                s1 += LTR_DPP(s1, LTR_DPP_HALF_MIRROR);
                s1 += LTR_DPP(s1, LTR_DPP_MIRROR);
                const float m = s1 / (float)F;
                float s2 = 0.f, dt = 0.f;
                for (int f = l; f < F; f += 16) {
                    const float c = x[f] - m;
                    s2 = fmaf(c, c, s2);
                    dt = fmaf(c, a.weff[f], dt);
                }
                s2 += LTR_DPP(s2, LTR_DPP_XOR1);
                s2 += LTR_DPP(s2, LTR_DPP_XOR2);
                s2 += LTR_DPP(s2, LTR_DPP_HALF_MIRROR);
                s2 += LTR_DPP(s2, LTR_DPP_MIRROR);
                dt += LTR_DPP(dt, LTR_DPP_XOR1);
                dt += LTR_DPP(dt, LTR_DPP_XOR2);
                dt += LTR_DPP(dt, LTR_DPP_HALF_MIRROR);
                dt += LTR_DPP(dt, LTR_DPP_MIRROR);
                const float rstd = 1.f / sqrtf(s2 / (float)F + kLnEps);
                if (l == 0) {
                    sc[d] = fmaf(rstd, dt, a.weff[F]);
                    mu[d] = m;
                    rs[d] = rstd;
                }
            } else {
                float dt = 0.f;
                for (int c = l; c < F4; c += 16) {
                    const float4 v = *reinterpret_cast<const float4 *>(x + 4 * c);
                    const float4 w = reinterpret_cast<const float4 *>(a.weff)[c];
                    dt = fmaf(v.x, w.x, dt);
                    dt = fmaf(v.y, w.y, dt);
                    dt = fmaf(v.z, w.z, dt);
                    dt = fmaf(v.w, w.w, dt);
                }
                dt += LTR_DPP(dt, LTR_DPP_XOR1);
                dt += LTR_DPP(dt, LTR_DPP_XOR2);
                dt += LTR_DPP(dt, LTR_DPP_HALF_MIRROR);
                dt += LTR_DPP(dt, LTR_DPP_MIRROR);
                if (l == 0) sc[d] = dt + a.weff[F];
            }
        }
        __syncthreads();
        // slate state of group gid: slate b = tile * gpb + gid, documents [gid * S, gid * S + S) of the tile
        const long long slate = tile * gpb + gid;
        const bool active = slate < a.B;
        const SlateGroup g = make_group(S, group, gb + kLossArrays * S, tid);
        float *s0 = gb, *s1 = gb + S;
        for (int j = g.t; j < S; j += group) {
            const float y = active ? a.labels[slate * S + j] : a.pad;
            const float s = active ? sc[gid * S + j] : 0.f;
            s0[j] = LK == 1 ? y : s;                              // ListNet: yt, yp;  others: sc, yl, gn
            if (LK == 1) {
                s1[j] = s;
            } else {
                stage_label(y, a.pad, s1[j], gb[2 * S + j]);
            }
        }
        __syncthreads();
        float *dd = dsl + gid * S;
        auto store = [&](int i, float v) { if (active) dd[i] = v; };
        float loss;
        if (LK == 0) {
            ApproxScratch xsr;
            xsr.um = gb + 6 * S;
            loss = approx_ndcg_slate(g, gb, gb + S, gb + 2 * S, gb + 3 * S, gb + 4 * S, gb + 5 * S, a.alpha, a.eps, a.gscale, true,
                                     store, NoStamp(), xsr);
        } else if (LK == 1) {
            loss = listnet_slate(g, s0, s1, a.apply_sigmoid != 0, a.gscale, true, store);
        } else {
            LambdaLds L;
            L.sc = gb;
            L.yl = gb + S;
            L.gn = gb + 2 * S;
            L.w1 = gb + 3 * S;
            L.invd = gb + 4 * S;
            L.delta = gb + 5 * S;
            L.rk = reinterpret_cast<int *>(gb + 6 * S);
            float count;
            loss = lambda_slate<SCH>(g, L, a.lp, a.gscale, true, &count, store);
            if (active && g.t == 0 && a.slate_count) a.slate_count[slate] = count;
        }
        if (active && g.t == 0) a.slate_loss[slate] = loss;
        __syncthreads();
        if (tid < F) {
            if (LN) {
                for (int d = 0; d < kTile; ++d) acc = fmaf(dsl[d] * rs[d], xs[d * LD + tid] - mu[d], acc);
            } else {
                for (int d = 0; d < kTile; ++d) acc = fmaf(dsl[d], xs[d * LD + tid], acc);
            }
        }
        for (int d = 0; d < kTile; ++d) g1 += dsl[d];
    }
    float *out = a.partials + (size_t)blockIdx.x * (F + 1);
    if (tid < F) out[tid] = acc;
    if (tid == 0) out[F] = g1;
}

// ------------------------------------------------------------------------------------- risk-sensitive losses, Listnet forms
// The risk losses' value is not a sum over slates (riskLosses.py:8-49, :128-169, :247-276 feed a batch-wide tail), but entry mat[q][0]
// of their effectiveness matrix depends on slate q's scores alone.  With j_d = d mat[q][0] / d s_d and c_q = d value / d mat[q][0],
//     [Ghat | G_1] = sum_q c_q R_q,      R_q = [ sum_d j_d xhat_d | sum_d j_d ]        (F + 1 floats per slate, known BEFORE the tail)
// so X is read once: linear_risk_rows_kernel (linear_fused_kernel's tile loop) leaves mat[:, 0] and R, the tail runs on the matrix, and
// linear_risk_combine_kernel forms the partials ltr_linear_unfold_grads reduces.
//
// The per-slate function restates risk_matrix_kernel modes 0 and 2 (ltr_risk.hip): the slate softmaxes, transformations 1 / 2 / 3 against
// the labels, fp32 elementwise, fp64 sums, the per-norm cosine clamp with the gradient through the unclamped norm.  It is NOT shared with
// that kernel: there a 256-thread workgroup strides one slate held in LDS, here 2 S threads hold one document each in registers, and
// sharing one function would change that kernel's summation order, whose results stay bit-for-bit as they are.
struct RiskRowsArgs {
    const float *X, *labels, *weff, *cached;
    int B, S, F, mode, lt, n_cached, cache_stride, nsys;
    float *mat, *R;
};

inline size_t risk_rows_lds_bytes(int F) {
    return ((size_t)kTile * (F + 4) + 4 * kTile) * sizeof(float) + 4 * 8 * sizeof(double);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;   // butterfly: every lane holds the same bits
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// v[0 .. N) summed (MAX: maximised) over the wps waves of a slate group, first wave w0; every thread gets the result.  Lanes by
// butterfly, waves in order.  All threads of the block call it.
template <int N, bool MAX>
__device__ __forceinline__ void slate_reduce(double (&v)[N], double *red /* [4][8] */, int w0, int wps) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = MAX ? (double)wave_max_f32((float)v[k]) : wave_sum_f64(v[k]);
    if (wps == 1) return;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[wave * 8 + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = red[w0 * 8 + k];
        for (int w = 1; w < wps; ++w) s = MAX ? fmax(s, red[(w0 + w) * 8 + k]) : s + red[(w0 + w) * 8 + k];
        v[k] = s;
    }
}

template <bool LN>
__global__ void __launch_bounds__(256) linear_risk_rows_kernel(RiskRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = a.F, S = a.S, LD = F + 4, F4 = F >> 2, F1 = F + 1;
    float *xs = smem;                          // [128][LD]
    float *sc = xs + kTile * LD;               // [128] scores
    float *jl = sc + kTile;                    // [128] d mat[q][0] / d s
    float *mu = jl + kTile;                    // [128] row mean      (input_norm)
    float *rs = mu + kTile;                    // [128] row 1 / std   (input_norm)
    double *red = reinterpret_cast<double *>(rs + kTile);   // [4 waves][8]  (byte offset 512 (F + 4) + 2048: 8-byte aligned)
    const int group = 2 * S, gpb = kTile / S, wps = group >> 6;    // S in {32, 64, 128}: 1, 2, 4 waves per slate
    const int tid = threadIdx.x;
    const int gid = tid / group, t = tid - gid * group, w0 = gid * wps;
    const long long n = (long long)a.B * S;
    const long long tiles = (n + kTile - 1) / kTile;
    const int r = tid >> 4, l = tid & 15;      // DPP row r scores documents r, r + 16, ...
    const int mode = a.mode, lt = a.lt;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();                       // previous tile's LDS reads done
        const long long base = tile * kTile;
        const int nd = (int)(n - base < kTile ? n - base : kTile);
        const float4 *src = reinterpret_cast<const float4 *>(a.X + base * F);
        for (int q = tid; q < kTile * F4; q += 256) {
            const int d = q / F4, c = q - d * F4;
            const float4 v = d < nd ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(xs + d * LD + 4 * c) = v;
        }
        __syncthreads();
        for (int d = r; d < kTile; d += 16) {
            const float *x = xs + d * LD;
            if (LN) {
                float s1 = 0.f;
                for (int f = l; f < F; f += 16) s1 += x[f];
                s1 += LTR_DPP(s1, LTR_DPP_XOR1);
                s1 += LTR_DPP(s1, LTR_DPP_XOR2);
                s1 += LTR_DPP(s1, LTR_DPP_HALF_MIRROR);
                s1 += LTR_DPP(s1, LTR_DPP_MIRROR);
                const float m = s1 / (float)F;
                float s2 = 0.f, dt = 0.f;
                for (int f = l; f < F; f += 16) {
                    const float c = x[f] - m;
                    s2 = fmaf(c, c, s2);
                    dt = fmaf(c, a.weff[f], dt);
                }
                s2 += LTR_DPP(s2, LTR_DPP_XOR1);
                s2 += LTR_DPP(s2, LTR_DPP_XOR2);
                s2 += LTR_DPP(s2, LTR_DPP_HALF_MIRROR);
                s2 += LTR_DPP(s2, LTR_DPP_MIRROR);
                dt += LTR_DPP(dt, LTR_DPP_XOR1);
                dt += LTR_DPP(dt, LTR_DPP_XOR2);
                dt += LTR_DPP(dt, LTR_DPP_HALF_MIRROR);
                dt += LTR_DPP(dt, LTR_DPP_MIRROR);
                const float rstd = 1.f / sqrtf(s2 / (float)F + kLnEps);
                if (l == 0) {
                    sc[d] = fmaf(rstd, dt, a.weff[F]);
                    mu[d] = m;
                    rs[d] = rstd;
                }
            } else {
                float dt = 0.f;
                for (int c = l; c < F4; c += 16) {
                    const float4 v = *reinterpret_cast<const float4 *>(x + 4 * c);
                    const float4 w = reinterpret_cast<const float4 *>(a.weff)[c];
                    dt = fmaf(v.x, w.x, dt);
                    dt = fmaf(v.y, w.y, dt);
                    dt = fmaf(v.z, w.z, dt);
                    dt = fmaf(v.w, w.w, dt);
                }
                dt += LTR_DPP(dt, LTR_DPP_XOR1);
                dt += LTR_DPP(dt, LTR_DPP_XOR2);
                dt += LTR_DPP(dt, LTR_DPP_HALF_MIRROR);
                dt += LTR_DPP(dt, LTR_DPP_MIRROR);
                if (l == 0) sc[d] = dt + a.weff[F];
            }
        }
        __syncthreads();
        // slate b = tile * gpb + gid: documents [gid * S, gid * S + S) of the tile, document t held by thread t of the group (t < S)
        const long long slate = tile * gpb + gid;
        const bool active = slate < a.B, own = active && t < S;
        if (active)                            // the constant systems' entries, copied next to the model's
            for (int k = t; k < a.n_cached; k += group) a.mat[slate * a.nsys + 1 + k] = a.cached[slate * a.cache_stride + k];
        const float yl = own ? a.labels[slate * S + t] : 0.f, sv = own ? sc[gid * S + t] : 0.f;
        double mx[2] = {own ? (double)yl : -INFINITY, own ? (double)sv : -INFINITY};
        slate_reduce<2, true>(mx, red, w0, wps);
        const float et = own ? expf(yl - (float)mx[0]) : 0.f, ex = own ? expf(sv - (float)mx[1]) : 0.f;
        double z[2] = {(double)et, (double)ex};
        slate_reduce<2, false>(z, red, w0, wps);
        const float tj = active ? et * (float)(1.0 / z[0]) : 0.f, xj = active ? ex * (float)(1.0 / z[1]) : 0.f;   // the two softmaxes
        const float df = tj * xj - tj * tj, u = tj * tj, v = tj * xj;
        double sm[7] = {(double)tj * tj, (double)tj * xj, (double)xj * xj, (double)df * df, (double)u * v, (double)u * u, (double)v * v};
        slate_reduce<7, false>(sm, red, w0, wps);
        const double nt = sm[0], aa = sm[1], nx = sm[2], cc = sm[3];
        // cosine operands (u, v) = (t, x) [mode 0] or the products (t^2, t x) [mode 2, riskLosses.py:256-258]; nn.CosineSimilarity clamps
        // EACH norm at eps = 1e-8 for the value while the gradient flows through the unclamped norm (risk_matrix_kernel)
        const double ca = mode == 2 ? sm[4] : aa, cnu = mode == 2 ? sm[5] : nt, cnv = mode == 2 ? sm[6] : nx;
        const double nrm_u = sqrt(cnu), nrm_v = sqrt(cnv);
        const double den = (nrm_u > 1e-8 ? nrm_u : 1e-8) * (nrm_v > 1e-8 ? nrm_v : 1e-8);
        double m;
        if (lt == 1) m = cc;
        else if (lt == 2) m = active ? ca / den : 0.0;
        else m = (aa - nt) * (aa - nt);
        const double nv_c = nrm_v > 1e-8 ? nrm_v : 1e-8;
        const double inv_vv = nrm_v > 0.0 ? 1.0 / (nv_c * nrm_v) : 0.0;
        double g;                              // d m / d x_j
        {
            const double td = tj, xd = xj;
            if (lt == 1) g = 2.0 * td * (td * xd - td * td);
            else if (lt == 2) {
                const double uu = mode == 2 ? td * td : td, vv = mode == 2 ? td * xd : xd, ww = mode == 2 ? td : 1.0;
                g = ww * (uu / den - m * vv * inv_vv);
            } else g = 2.0 * (aa - nt) * td;
        }
        double dot[1] = {own ? (double)xj * g : 0.0};
        slate_reduce<1, false>(dot, red, w0, wps);
        // x = softmax(s): d m / d s_j = x_j (g_j - sum_k x_k g_k)
        if (t < S) jl[gid * S + t] = own ? (float)((double)xj * (g - dot[0])) : 0.f;
        if (active && t == 0) a.mat[slate * a.nsys] = (float)m;
        __syncthreads();
        // R_q = [sum_d j_d xhat_d | sum_d j_d] from the same LDS rows, thread f owning feature f, documents in order
        if (tid < F) {
            for (int gq = 0; gq < gpb; ++gq) {
                const long long q = tile * gpb + gq;
                if (q >= a.B) break;
                float acc = 0.f, g1 = 0.f;
                const int d0 = gq * S;
                if (LN) {
                    for (int d = d0; d < d0 + S; ++d) {
                        acc = fmaf(jl[d] * rs[d], xs[d * LD + tid] - mu[d], acc);
                        g1 += jl[d];
                    }
                } else {
                    for (int d = d0; d < d0 + S; ++d) {
                        acc = fmaf(jl[d], xs[d * LD + tid], acc);
                        g1 += jl[d];
                    }
                }
                a.R[q * F1 + tid] = acc;
                if (tid == 0) a.R[q * F1 + F] = g1;
            }
        }
    }
}

// partials[g] = sum_{q in range(g)} c_q R_q, c_q = dmat[q * dmat_stride]; workgroup g takes a contiguous range of slates, thread f
// column f, slates in order.  Every workgroup writes its row (zeros for an empty range): the unfold reduces all `grid` rows.
__global__ void __launch_bounds__(256) linear_risk_combine_kernel(const float *__restrict__ R, const float *__restrict__ dmat,
                                                                  int dmat_stride, int B, int F1, float *__restrict__ partials) {
    const int per = (B + (int)gridDim.x - 1) / (int)gridDim.x;
    const long long q0 = (long long)blockIdx.x * per;
    const long long q1 = q0 + per < B ? q0 + per : B;
    for (int f = threadIdx.x; f < F1; f += 256) {
        float acc = 0.f;
        for (long long q = q0; q < q1; ++q) acc = fmaf(dmat[q * dmat_stride], R[q * F1 + f], acc);
        partials[(size_t)blockIdx.x * F1 + f] = acc;
    }
}

template <int LK, int SCH, bool LN>
int launch_fused(const FusedArgs &a, int grid, hipStream_t stream) {
    const size_t lds = fused_lds_bytes(a.F, a.S);
    if (int rc = allow_lds(linear_fused_kernel<LK, SCH, LN>, lds)) return rc;
    hipLaunchKernelGGL((linear_fused_kernel<LK, SCH, LN>), dim3(grid), dim3(256), lds, stream, a);
    return launch_status();
}

template <int LK, int SCH>
int launch_fused_ln(const FusedArgs &a, int ln, int grid, hipStream_t stream) {
    return ln ? launch_fused<LK, SCH, true>(a, grid, stream) : launch_fused<LK, SCH, false>(a, grid, stream);
}

}  // namespace

extern "C" {

int64_t ltr_linear_ws_doubles(int n_layers, int F, const int *sizes) {
    if (n_layers < 0 || n_layers > kLinMaxLayers || F < 1 || (n_layers > 0 && !sizes)) return -1;
    int64_t s = F;
    for (int i = 0; i < n_layers; ++i) s += sizes[i];
    return 2 * s + F + 1;
}

int ltr_linear_fold(int n_layers, int F, const int *sizes, int input_norm, const float *const *params, double *ws, float *weff,
                    void *stream) {
    LinNet N;
    if (int rc = make_net(n_layers, F, sizes, input_norm, params, N)) return rc;
    if (!ws || !weff) return LTR_ERR_NULL;
    hipLaunchKernelGGL(linear_fold_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, N, ws, weff);
    return launch_status();
}

int ltr_linear_unfold_grads(int n_layers, int F, const int *sizes, int input_norm, const float *const *params, const float *partials,
                            int grid, double *ws, float *flat, void *stream) {
    LinNet N;
    if (int rc = make_net(n_layers, F, sizes, input_norm, params, N)) return rc;
    if (!partials || !ws || !flat) return LTR_ERR_NULL;
    if (grid < 1) return LTR_ERR_PARAM;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(linear_reduce_partials_kernel, dim3((F + 1 + 63) / 64), dim3(1024), 0, s, partials, grid, F + 1, ws + N.go);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(linear_unfold_kernel, dim3(1), dim3(1024), 0, s, N, ws, flat);
    if (int rc = launch_status()) return rc;
    if (N.nW > 0) {
        hipLaunchKernelGGL(linear_outer_kernel, ltr_grid((N.nW + 255) / 256), dim3(256), 0, s, N, ws, flat);
        return launch_status();
    }
    return LTR_OK;
}

int ltr_linear_scores(const float *X, int64_t n, int F, const float *weff, int input_norm, float *scores, float *stats, void *stream) {
    if (!X || !weff || !scores || (input_norm && !stats)) return LTR_ERR_NULL;
    if (n < 0 || F < 1 || F > kLinMaxF) return LTR_ERR_SHAPE;
    if (input_norm != 0 && input_norm != 1) return LTR_ERR_PARAM;
    if (n == 0) return LTR_OK;
    const bool vec = F % 4 == 0 && ((uintptr_t)X % 16) == 0 && ((uintptr_t)weff % 16) == 0;
    const dim3 grid = ltr_grid((n + 15) / 16);
    hipStream_t s = (hipStream_t)stream;
    if (input_norm) {
        if (vec) hipLaunchKernelGGL((linear_scores_kernel<true, true>), grid, dim3(256), 0, s, X, n, F, weff, scores, stats);
        else hipLaunchKernelGGL((linear_scores_kernel<false, true>), grid, dim3(256), 0, s, X, n, F, weff, scores, stats);
    } else {
        if (vec) hipLaunchKernelGGL((linear_scores_kernel<true, false>), grid, dim3(256), 0, s, X, n, F, weff, scores, stats);
        else hipLaunchKernelGGL((linear_scores_kernel<false, false>), grid, dim3(256), 0, s, X, n, F, weff, scores, stats);
    }
    return launch_status();
}

int ltr_linear_grad_partials(const float *X, int64_t n, int F, const float *dscores, const float *stats, int input_norm, float *partials,
                             int grid, void *stream) {
    if (!X || !dscores || !partials || (input_norm && !stats)) return LTR_ERR_NULL;
    if (n < 0 || F < 1 || F > kLinMaxF) return LTR_ERR_SHAPE;
    if (input_norm != 0 && input_norm != 1) return LTR_ERR_PARAM;
    if (grid < 1) return LTR_ERR_PARAM;
    hipStream_t s = (hipStream_t)stream;
    if (input_norm)
        hipLaunchKernelGGL(linear_grad_partials_kernel<true>, dim3(grid), dim3(256), 0, s, X, (long long)n, F, dscores, stats, partials);
    else
        hipLaunchKernelGGL(linear_grad_partials_kernel<false>, dim3(grid), dim3(256), 0, s, X, (long long)n, F, dscores, stats, partials);
    return launch_status();
}

int ltr_linear_fused_supported(int F, int S) {
    return (S == 32 || S == 64 || S == 128) && F >= 4 && F <= kLinFusedMaxF && F % 4 == 0;
}

int ltr_linear_fused_step(int loss_kind, const float *X, const float *labels, int B, int S, int F, const float *weff, int input_norm,
                          float alpha, float eps, float pad, int apply_sigmoid, int scheme, int k, float sigma, float mu,
                          float lambda_eps, int log_base, float grad_scale, float *slate_loss, float *slate_count, float *partials,
                          int grid, void *stream) {
    if (!X || !labels || !weff || !slate_loss || !partials) return LTR_ERR_NULL;
    if (B < 0 || !ltr_linear_fused_supported(F, S)) return LTR_ERR_SHAPE;
    if ((uintptr_t)X % 16 || (uintptr_t)weff % 16) return LTR_ERR_ALIGN;
    if (loss_kind < 0 || loss_kind > 2 || grid < 1 || (input_norm != 0 && input_norm != 1)) return LTR_ERR_PARAM;
    FusedArgs a;
    a.X = X;
    a.labels = labels;
    a.weff = weff;
    a.B = B;
    a.S = S;
    a.F = F;
    a.alpha = alpha;
    a.eps = eps;
    a.pad = pad;
    a.gscale = grad_scale;
    a.apply_sigmoid = apply_sigmoid;
    a.slate_loss = slate_loss;
    a.slate_count = slate_count;
    a.partials = partials;
    a.lp = LambdaParams{};
    hipStream_t s = (hipStream_t)stream;
    if (loss_kind == 0) return launch_fused_ln<0, 0>(a, input_norm, grid, s);
    if (loss_kind == 1) return launch_fused_ln<1, 0>(a, input_norm, grid, s);
    if (scheme < 0 || scheme > 7 || (log_base != LTR_LOG_BINARY && log_base != LTR_LOG_NATURAL) || !(lambda_eps > 0.f))
        return LTR_ERR_PARAM;
    a.lp.scheme = scheme;
    a.lp.k = k;
    a.lp.sigma = sigma;
    a.lp.mu = mu;
    a.lp.eps = lambda_eps;
    a.lp.log_scale = log_base == LTR_LOG_BINARY ? (float)(1.0 / 0.693147180559945309417) : 1.f;
    a.lp.log_floor = log_base == LTR_LOG_BINARY ? log2f(lambda_eps) : logf(lambda_eps);
    switch (scheme) {
        case 0: return launch_fused_ln<2, 0>(a, input_norm, grid, s);
        case 1: return launch_fused_ln<2, 1>(a, input_norm, grid, s);
        case 2: return launch_fused_ln<2, 2>(a, input_norm, grid, s);
        case 3: return launch_fused_ln<2, 3>(a, input_norm, grid, s);
        case 4: return launch_fused_ln<2, 4>(a, input_norm, grid, s);
        case 5: return launch_fused_ln<2, 5>(a, input_norm, grid, s);
        case 6: return launch_fused_ln<2, 6>(a, input_norm, grid, s);
        default: return launch_fused_ln<2, 7>(a, input_norm, grid, s);
    }
}

int ltr_linear_risk_rows(const float *X, const float *labels, int B, int S, int F, const float *weff, int input_norm, int mode, int lt,
                         const float *cached, int cache_stride, int n_cached, float *mat, int n_systems, float *R, int grid,
                         void *stream) {
    if (!X || !labels || !weff || !mat || !R || (n_cached > 0 && !cached)) return LTR_ERR_NULL;
    if (B < 1 || !ltr_linear_fused_supported(F, S) || n_cached < 0 || n_cached > 65 || cache_stride < n_cached ||
        n_systems < 1 + n_cached)
        return LTR_ERR_SHAPE;
    if ((uintptr_t)X % 16 || (uintptr_t)weff % 16) return LTR_ERR_ALIGN;
    if ((mode != 0 && mode != 2) || lt < 1 || lt > 3 || grid < 1 || grid > LTR_GRID_X_MAX || (input_norm != 0 && input_norm != 1))
        return LTR_ERR_PARAM;
    RiskRowsArgs a;
    a.X = X;
    a.labels = labels;
    a.weff = weff;
    a.cached = cached;
    a.B = B;
    a.S = S;
    a.F = F;
    a.mode = mode;
    a.lt = lt;
    a.n_cached = n_cached;
    a.cache_stride = cache_stride;
    a.nsys = n_systems;
    a.mat = mat;
    a.R = R;
    const long long tiles = ((long long)B * S + kTile - 1) / kTile;
    if (grid > tiles) grid = (int)tiles;
    const size_t lds = risk_rows_lds_bytes(F);
    hipStream_t s = (hipStream_t)stream;
    if (input_norm) {
        if (int rc = allow_lds(linear_risk_rows_kernel<true>, lds)) return rc;
        hipLaunchKernelGGL(linear_risk_rows_kernel<true>, ltr_grid(grid), dim3(256), lds, s, a);
    } else {
        if (int rc = allow_lds(linear_risk_rows_kernel<false>, lds)) return rc;
        hipLaunchKernelGGL(linear_risk_rows_kernel<false>, ltr_grid(grid), dim3(256), lds, s, a);
    }
    return launch_status();
}

int ltr_linear_risk_combine(const float *R, const float *dmat, int dmat_stride, int B, int F, float *partials, int grid, void *stream) {
    if (!R || !dmat || !partials) return LTR_ERR_NULL;
    if (B < 1 || F < 1 || F > kLinMaxF || dmat_stride < 1) return LTR_ERR_SHAPE;
    if (grid < 1 || grid > LTR_GRID_X_MAX) return LTR_ERR_PARAM;
    hipLaunchKernelGGL(linear_risk_combine_kernel, ltr_grid(grid), dim3(256), 0, (hipStream_t)stream, R, dmat, dmat_stride, B, F + 1,
                       partials);
    return launch_status();
}

int ltr_linear_grid(int n_cus) {
    return n_cus < 1 ? 1 : 2 * n_cus;
}

}  // extern "C"
