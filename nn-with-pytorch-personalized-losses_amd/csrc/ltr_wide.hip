// ltr_wide.hip -- FC scorers with MORE than 136 input features (Istella: 220, Yahoo LTRC: 700), 137 .. 1024 (gfx950 / MI355X).
//
// Replaces, for those widths:
//   architeture/doubleLayer.py:54-73  DoubleLayerNet  fc3(drop(relu(fc2(drop(relu(fc1 x))))))          LTR_WIDE_RELU3
//   architeture/tripleLayer.py:5-17   TripleLayerNet  l3(sigmoid(l2(l1 x))), l2 . l1 folded (ltr_triple_fold)  LTR_WIDE_SIGMOID2
//
// The slate pipeline (ltr_scorer.hip) keeps a 128-document fp32 tile of the input in LDS, which stops at 136 features.  Here every
// layer is a plain tiled GEMM on v_mfma_f32_16x16x4_f32 (exact fp32: each output is a k-ordered fmaf chain) with the scorers'
// epilogues, and the training step is a CHAIN of launches around saved post-activation layers, like ltr_mlp_forward_save /
// ltr_mlp_backward_saved:
//   * ltr_gemm_f32: 64 x 64 output tile per 256-thread workgroup, 16-wide k tiles staged through LDS as [k][row] images of row stride
//     80 floats (the four k rows of one MFMA step fall 16 banks apart: conflict-free fragment reads), the next k tile prefetched into
//     registers while the current one multiplies.  Wave w owns the 32 x 32 quarter (w >> 1, w & 1): 2 x 2 accumulator tiles, four
//     independent MFMA chains.  Operands are read where they lie (k-major flags), 16 bytes per lane where base and leading dimension
//     allow it and 4 bytes otherwise; rows and k outside the extents are zero-filled in LDS and never read.
//   * split over K for the weight gradients (K = documents): slice z writes its raw partial, ltr_enc_sum_partials adds the slices in
//     a fixed order with an fp64 accumulator.  No float atomics anywhere: the same inputs give the same bits.
//   * ltr_colsum_f32 (bias gradients, and d w3 with the rows weighted by d loss / d score), a row-dot kernel for the last layer.
// This file has no LTR_F16X2 branch: both libraries compile the same exact-fp32 code.
#include "../../include/ltr_encoder.h"
#include "../../include/ltr_mi355x.h"
#include "ltr_device.h"
#include <string.h>

using namespace ltr;

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kBM = 64, kBN = 64, kBK = 16;    // output tile and k tile of one workgroup (tests/wide_cases.py walks their edges)
constexpr int kLd = 80;                        // LDS row stride in floats: 4 k rows x 16 lanes land in 64 distinct banks
constexpr int kThreads = 256;
constexpr int kMaxWidth = 1024;
constexpr int kMaxSplits = 1024;

struct GemmArgs {
    const float *A, *B;
    long long M, N, K, lda, ldb, ldc;
    long long tiles_m, kchunk;       // kchunk: k per slice, a multiple of kBK
    int tiles_n, splits;
    int a_vec, b_vec;                // 16-byte loads allowed for the operand
    float *C;
    const float *bias;
    int act;                         // LTR_GEMM_ACT_*
    const float *gate;
    long long ldg;
    int gate_kind;                   // LTR_GEMM_GATE_*
    float gate_scale;
    int drop_on;
    unsigned thr16;                  // 0: p = 0.5, one hash bit per unit; else 16 bits per unit (stream layer + 2)
    float drop_scale;
    unsigned long long seed;
    int layer;
    const uint8_t *keep;             // explicit keep mask [M][N] (bytes), used INSTEAD of the stream
};

// Four consecutive elements of one operand tile -> registers, zero where (row, k) is outside the extents.
//   KM = false: element (row, k) at P[row * ld + k]; the four are k .. k + 3 of one row.
//   KM = true:  element (row, k) at P[k * ld + row]; the four are row .. row + 3 of one k.
template <bool KM>
__device__ __forceinline__ f32x4 load_quad(const float *__restrict__ P, long long ld, long long row, long long rows, long long k,
                                           long long k_end, int vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!KM) {
        if (row >= rows) return v;
        const float *p = P + row * ld + k;
        if (vec && k + 3 < k_end) return *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + j < k_end) v[j] = p[j];
    } else {
        if (k >= k_end) return v;
        const float *p = P + k * ld + row;
        if (vec && row + 3 < rows) return *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (row + j < rows) v[j] = p[j];
    }
    return v;
}

// Thread t's quad of a 64-row x 16-k tile: KM = false -> row t / 4, k quad t % 4; KM = true -> k t / 16, row quad t % 16.
template <bool KM>
__device__ __forceinline__ f32x4 load_tile(const float *__restrict__ P, long long ld, long long row0, long long rows, long long k0,
                                           long long k_end, int vec, int t) {
    if (!KM) return load_quad<false>(P, ld, row0 + (t >> 2), rows, k0 + 4 * (t & 3), k_end, vec);
    return load_quad<true>(P, ld, row0 + 4 * (t & 15), rows, k0 + (t >> 4), k_end, vec);
}
template <bool KM>
__device__ __forceinline__ void store_tile(float *S /* [kBK][kLd] */, f32x4 v, int t) {
    if (!KM) {
#pragma unroll
        for (int j = 0; j < 4; ++j) S[(4 * (t & 3) + j) * kLd + (t >> 2)] = v[j];
    } else {
        *reinterpret_cast<f32x4 *>(S + (t >> 4) * kLd + 4 * (t & 15)) = v;
    }
}

__device__ __forceinline__ bool keep_unit(const GemmArgs &g, long long m, int n) {
    if (g.keep) return g.keep[m * g.N + n] != 0;
    if (g.thr16) return ((keep_word(g.seed, g.layer + 2, m, n >> 1) >> (16 * (n & 1))) & 0xffffu) >= g.thr16;
    return (keep_word(g.seed, g.layer, m, n >> 5) >> (n & 31)) & 1u;
}

template <bool AKM, bool BKM>
__global__ void __launch_bounds__(kThreads) gemm_f32_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[kBK * kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * kLd];
    const long long id = ltr_block_id();
    const long long per_slice = g.tiles_m * g.tiles_n;
    if (id >= per_slice * g.splits) return;           // workgroup-uniform, before the first barrier
    const long long z = id / per_slice, rem = id - z * per_slice;
    const long long tm = rem / g.tiles_n;
    const int tn = (int)(rem - tm * g.tiles_n);
    const long long m0 = tm * kBM, n0 = (long long)tn * kBN;
    const long long k_begin = z * g.kchunk;
    const long long k_end = k_begin + g.kchunk < g.K ? k_begin + g.kchunk : g.K;
    const long long nkt = k_end > k_begin ? (k_end - k_begin + kBK - 1) / kBK : 0;     // a slice past the end of K: zeros

    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int wm = 32 * (w >> 1), wn = 32 * (w & 1);
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 ra = {0.f, 0.f, 0.f, 0.f}, rb = ra;
    if (nkt > 0) {
        ra = load_tile<AKM>(g.A, g.lda, m0, g.M, k_begin, k_end, g.a_vec, t);
        rb = load_tile<BKM>(g.B, g.ldb, n0, g.N, k_begin, k_end, g.b_vec, t);
    }
    for (long long kt = 0; kt < nkt; ++kt) {          // nkt is workgroup-uniform: both barriers are reached by every thread
        store_tile<AKM>(As, ra, t);
        store_tile<BKM>(Bs, rb, t);
        __syncthreads();
        if (kt + 1 < nkt) {
            const long long kn = k_begin + (kt + 1) * kBK;
            ra = load_tile<AKM>(g.A, g.lda, m0, g.M, kn, k_end, g.a_vec, t);
            rb = load_tile<BKM>(g.B, g.ldb, n0, g.N, kn, k_end, g.b_vec, t);
        }
#pragma unroll
        for (int s = 0; s < kBK / 4; ++s) {
            const float *ar = As + (4 * s + q) * kLd + wm + i, *br = Bs + (4 * s + q) * kLd + wn + i;
            const float a0 = ar[0], a1 = ar[16], b0 = br[0], b1 = br[16];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    // accumulator tile (a, b): row = 4 q + r, column = i
    float *C = g.C + (g.splits > 1 ? z * g.M * g.ldc : 0);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = m0 + wm + 16 * a + 4 * q + r;
            if (m >= g.M) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const long long nn = n0 + wn + 16 * b + i;
                if (nn >= g.N) continue;
                const int n = (int)nn;
                float v = acc[a][b][r];
                if (g.splits == 1) {
                    if (g.bias) v = v + g.bias[n];
                    if (g.act == LTR_GEMM_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (g.act == LTR_GEMM_ACT_SIGMOID) v = __frcp_rn(1.f + __expf(-v));
                    if (g.gate_kind == LTR_GEMM_GATE_RELU) {
                        v = g.gate[m * g.ldg + n] > 0.f ? v * g.gate_scale : 0.f;
                    } else if (g.gate_kind == LTR_GEMM_GATE_SIGMOID) {
                        const float h = g.gate[m * g.ldg + n];
                        v = v * (h * (1.f - h));
                    }
                    if (g.drop_on) v = keep_unit(g, m, n) ? v * g.drop_scale : 0.f;
                }
                C[m * g.ldc + n] = v;
            }
        }
    }
}

// partials[blk][n] = sum over workgroup blk's contiguous row range of w[t] * y[t][n] (w == NULL: 1).  Wave v takes rows v, v + 4, ...
// of the range, 64 columns at a time (one 256-byte row segment per load); the four waves' sums meet in LDS in a fixed order.
__global__ void __launch_bounds__(kThreads) colsum_f32_kernel(const float *__restrict__ y, long long T, int N, long long ld,
                                                               const float *__restrict__ wt, float *__restrict__ partials) {
    __shared__ float red[4][64];
    const long long nblk = gridDim.x, blk = blockIdx.x;
    const long long per = (T + nblk - 1) / nblk;
    const long long r0 = blk * per, r1 = r0 + per < T ? r0 + per : T;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c0 = 0; c0 < N; c0 += 64) {               // N is uniform: every thread reaches both barriers of every pass
        const int c = c0 + lane;
        float s = 0.f;
        if (c < N) {
#pragma unroll 4
            for (long long r = r0 + wv; r < r1; r += 4) {
                const float v = y[r * ld + c];
                s += wt ? wt[r] * v : v;
            }
        }
        red[wv][lane] = s;
        __syncthreads();
        if (wv == 0 && c < N) partials[blk * N + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        __syncthreads();
    }
}

// out[t] = w . y[t] + b[0]: one wave per row, lanes stride the columns, a symmetric butterfly adds the 64 lane sums.
__global__ void __launch_bounds__(kThreads) rowdot_f32_kernel(const float *__restrict__ y, long long T, int N, long long ld,
                                                               const float *__restrict__ w, const float *__restrict__ b,
                                                               float *__restrict__ out) {
    const long long row = ltr_block_id() * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int lane = threadIdx.x & 63;
    const float *p = y + row * ld;
    float s = 0.f;
    for (int c = lane; c < N; c += 64) s = fmaf(p[c], w[c], s);
    s = wave_allsum(s);
    if (lane == 0) out[row] = s + b[0];
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline long long r4(long long n) { return (n + 3) & ~3ll; }

// `dropout` of the launchers (include/ltr_mi355x.h: 0, 1 or 1 | bits of p) -> p; false where p is outside (0, 1).
inline bool decode_drop(int dropout, int &on, unsigned &thr16, float &scale) {
    on = dropout & 1;
    thr16 = 0;
    scale = 1.f;
    if (!on) return true;
    const unsigned bits = (unsigned)dropout & ~1u;
    float p = 0.5f;
    if (bits) memcpy(&p, &bits, sizeof p);
    if (!(p > 0.f && p < 1.f)) return false;
    thr16 = p == 0.5f ? 0u : (unsigned)(p * 65536.f + 0.5f);
    if (thr16 > 65535u) thr16 = 65535u;
    scale = 1.f / (1.f - p);
    return true;
}

// Slices of a weight-gradient GEMM (M x N outputs, K documents) for `grid` wanted workgroups: enough to fill them, never more than
// there are 64-document blocks.
inline int wide_splits(long long M, long long N, long long K, int grid) {
    const long long tiles = ((M + kBM - 1) / kBM) * ((N + kBN - 1) / kBN);
    long long s = (grid + tiles - 1) / tiles;
    const long long blocks = (K + 63) / 64;
    if (s > blocks) s = blocks;
    if (s > kMaxSplits) s = kMaxSplits;
    return s < 1 ? 1 : (int)s;
}

int gemm(const ltr_gemm_f32_desc &d, hipStream_t stream) {
    GemmArgs g{};
    g.A = d.A; g.B = d.B;
    g.M = d.M; g.N = d.N; g.K = d.K; g.lda = d.lda; g.ldb = d.ldb; g.ldc = d.ldc;
    g.tiles_m = (d.M + kBM - 1) / kBM;
    g.tiles_n = (int)((d.N + kBN - 1) / kBN);
    g.splits = d.splits;
    const long long ktiles = (d.K + kBK - 1) / kBK;
    g.kchunk = (ktiles + d.splits - 1) / d.splits * kBK;
    g.a_vec = aligned16(d.A) && d.lda % 4 == 0;
    g.b_vec = aligned16(d.B) && d.ldb % 4 == 0;
    g.C = d.C;
    g.bias = d.bias;
    g.act = d.act;
    g.gate = d.gate;
    g.ldg = d.ldg;
    g.gate_kind = d.gate ? d.gate_kind : LTR_GEMM_GATE_NONE;
    g.gate_scale = d.gate_scale;
    decode_drop(d.dropout, g.drop_on, g.thr16, g.drop_scale);
    g.seed = d.seed;
    g.layer = d.drop_layer;
    g.keep = d.keep;
    const dim3 grid = ltr_grid(g.tiles_m * g.tiles_n * g.splits);
    if (d.a_kmajor) {
        if (d.b_kmajor) hipLaunchKernelGGL((gemm_f32_kernel<true, true>), grid, dim3(kThreads), 0, stream, g);
        else hipLaunchKernelGGL((gemm_f32_kernel<true, false>), grid, dim3(kThreads), 0, stream, g);
    } else {
        if (d.b_kmajor) hipLaunchKernelGGL((gemm_f32_kernel<false, true>), grid, dim3(kThreads), 0, stream, g);
        else hipLaunchKernelGGL((gemm_f32_kernel<false, false>), grid, dim3(kThreads), 0, stream, g);
    }
    return launch_status();
}

int check_kind(int kind, int F, int H1, int H2, int64_t n_docs, int grid = 1) {
    const bool two = kind == LTR_WIDE_SIGMOID2;
    if (F < 1 || F > kMaxWidth || H1 < 1 || H1 > kMaxWidth || n_docs < 0 || grid < 1 || grid > 65535) return LTR_ERR_SHAPE;
    if (!two && (H2 < 1 || H2 > kMaxWidth)) return LTR_ERR_SHAPE;
    if (kind != LTR_WIDE_RELU3 && !two) return LTR_ERR_PARAM;
    return LTR_OK;
}

}  // namespace

extern "C" {

int ltr_gemm_f32(const ltr_gemm_f32_desc *desc, void *stream) {
    if (!desc || !desc->A || !desc->B || !desc->C) return LTR_ERR_NULL;
    const ltr_gemm_f32_desc &d = *desc;
    if (d.gate_kind != LTR_GEMM_GATE_NONE && !d.gate) return LTR_ERR_NULL;
    if (d.M < 0 || d.N < 1 || d.N > kMaxWidth || d.K < 1 || d.splits < 1 || d.splits > kMaxSplits) return LTR_ERR_SHAPE;
    if (d.lda < (d.a_kmajor ? d.M : d.K) || d.ldb < (d.b_kmajor ? d.N : d.K) || d.ldc < d.N) return LTR_ERR_SHAPE;
    if (d.gate_kind != LTR_GEMM_GATE_NONE && d.ldg < d.N) return LTR_ERR_SHAPE;
    if (d.act < LTR_GEMM_ACT_NONE || d.act > LTR_GEMM_ACT_SIGMOID || d.gate_kind < LTR_GEMM_GATE_NONE ||
        d.gate_kind > LTR_GEMM_GATE_SIGMOID || d.drop_layer < 0 || d.drop_layer > 1)
        return LTR_ERR_PARAM;
    {
        int on;
        unsigned thr;
        float sc;
        if (!decode_drop(d.dropout, on, thr, sc)) return LTR_ERR_PARAM;
    }
    if (((uintptr_t)d.A | (uintptr_t)d.B | (uintptr_t)d.C | (uintptr_t)d.bias | (uintptr_t)d.gate) & 3u) return LTR_ERR_ALIGN;
    if (d.M == 0) return LTR_OK;
    return gemm(d, (hipStream_t)stream);
}

int ltr_colsum_f32(const float *y, int64_t T, int N, int64_t ld, const float *row_weights, float *partials, int nblk, void *stream) {
    if (!y || !partials) return LTR_ERR_NULL;
    if (T < 0 || N < 1 || N > kMaxWidth || ld < N || nblk < 1 || nblk > 65535) return LTR_ERR_SHAPE;
    hipLaunchKernelGGL(colsum_f32_kernel, dim3(nblk), dim3(kThreads), 0, (hipStream_t)stream, y, (long long)T, N, (long long)ld,
                       row_weights, partials);
    return launch_status();
}

int64_t ltr_wide_acts_floats(int kind, int F, int H1, int H2, int64_t n_docs) {
    if (int rc = check_kind(kind, F, H1, H2, n_docs)) return rc;
    return kind == LTR_WIDE_SIGMOID2 ? r4(n_docs * H1) : r4(n_docs * H1) + r4(n_docs * H2);
}

int64_t ltr_wide_ws_floats(int kind, int F, int H1, int H2, int64_t n_docs, int grid) {
    if (int rc = check_kind(kind, F, H1, H2, n_docs, grid)) return rc;
    const long long docs = n_docs > 0 ? n_docs : 1;
    long long parts = (long long)wide_splits(H1, F, docs, grid) * H1 * F;
    long long hmax = H1;
    long long dz = r4(n_docs * H1);
    if (kind == LTR_WIDE_RELU3) {
        const long long p2 = (long long)wide_splits(H2, H1, docs, grid) * H2 * H1;
        parts = p2 > parts ? p2 : parts;
        hmax = H2 > H1 ? H2 : H1;
        dz += r4(n_docs * H2);
    }
    const long long cs = (long long)grid * hmax;
    return dz + r4(cs > parts ? cs : parts);
}

int ltr_wide_forward_save(int kind, int F, int H1, int H2, const float *X, int64_t n_docs, const float *const *params, int dropout,
                          uint64_t seed, const uint8_t *keep1, const uint8_t *keep2, float *scores, float *acts, void *stream) {
    if (!X || !params || !scores || !acts) return LTR_ERR_NULL;
    const int np = kind == LTR_WIDE_SIGMOID2 ? 4 : 6;
    if (kind == LTR_WIDE_SIGMOID2 || kind == LTR_WIDE_RELU3)
        for (int k = 0; k < np; ++k)
            if (!params[k]) return LTR_ERR_NULL;
    if (int rc = check_kind(kind, F, H1, H2, n_docs)) return rc;
    int on;
    unsigned thr;
    float sc;
    if (!decode_drop(dropout, on, thr, sc)) return LTR_ERR_PARAM;
    if (!aligned16(X) || !aligned16(acts)) return LTR_ERR_ALIGN;
    if (n_docs == 0) return LTR_OK;
    hipStream_t s = (hipStream_t)stream;
    ltr_gemm_f32_desc d{};
    d.A = X; d.lda = F; d.B = params[0]; d.ldb = F;
    d.M = n_docs; d.N = H1; d.K = F; d.ldc = H1; d.splits = 1;
    d.C = acts;
    d.bias = params[1];
    d.seed = seed;
    if (kind == LTR_WIDE_SIGMOID2) {
        d.act = LTR_GEMM_ACT_SIGMOID;
        if (int rc = gemm(d, s)) return rc;
        hipLaunchKernelGGL(rowdot_f32_kernel, ltr_grid((n_docs + 3) / 4), dim3(kThreads), 0, s, (const float *)acts, (long long)n_docs, H1,
                           (long long)H1, params[2], params[3], scores);
        return launch_status();
    }
    float *h2 = acts + r4(n_docs * H1);
    d.act = LTR_GEMM_ACT_RELU;
    d.dropout = dropout; d.drop_layer = 0; d.keep = keep1;
    if (int rc = gemm(d, s)) return rc;
    d.A = acts; d.lda = H1; d.B = params[2]; d.ldb = H1;
    d.N = H2; d.K = H1; d.ldc = H2;
    d.C = h2;
    d.bias = params[3];
    d.drop_layer = 1; d.keep = keep2;
    if (int rc = gemm(d, s)) return rc;
    hipLaunchKernelGGL(rowdot_f32_kernel, ltr_grid((n_docs + 3) / 4), dim3(kThreads), 0, s, (const float *)h2, (long long)n_docs, H2,
                       (long long)H2, params[4], params[5], scores);
    return launch_status();
}

int ltr_wide_backward_saved(int kind, int F, int H1, int H2, const float *X, int64_t n_docs, const float *const *params, int dropout,
                            const float *acts, const float *dscores, float *ws, int grid, float *flat_grad, void *stream) {
    if (!X || !params || !acts || !dscores || !ws || !flat_grad) return LTR_ERR_NULL;
    const bool two = kind == LTR_WIDE_SIGMOID2;
    if (two || kind == LTR_WIDE_RELU3)
        for (int k = 0; k < (two ? 4 : 6); ++k)
            if (!params[k]) return LTR_ERR_NULL;
    if (int rc = check_kind(kind, F, H1, H2, n_docs, grid)) return rc;
    int on;
    unsigned thr;
    float slope;
    if (!decode_drop(dropout, on, thr, slope)) return LTR_ERR_PARAM;
    if (!aligned16(X) || !aligned16(acts) || !aligned16(ws)) return LTR_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const long long n_par = two ? (long long)H1 * F + H1 + H1 + 1 : (long long)H1 * F + H1 + (long long)H2 * H1 + H2 + H2 + 1;
    if (n_docs == 0) {
        const hipError_t e = hipMemsetAsync(flat_grad, 0, sizeof(float) * n_par, s);
        return e == hipSuccess ? LTR_OK : (int)e;
    }
    const int Hl = two ? H1 : H2;                      // the layer in front of the scoring vector
    const float *hl = two ? acts : acts + r4(n_docs * H1);
    float *gW1 = flat_grad, *gb1 = gW1 + (long long)H1 * F;
    float *gW2 = gb1 + H1, *gb2 = two ? nullptr : gW2 + (long long)H2 * H1;
    float *gw3 = two ? gW2 : gb2 + H2, *gb3 = gw3 + Hl;
    float *dzl = ws;                                   // d loss / d (pre-activation of layer Hl) [n_docs][Hl]
    float *dz1 = two ? ws : ws + r4(n_docs * H2);
    float *parts = dz1 + r4(n_docs * H1);
    const float *w3 = params[two ? 2 : 4];

    auto colsum = [&](const float *y, int N, const float *wt, float *out) -> int {
        hipLaunchKernelGGL(colsum_f32_kernel, dim3(grid), dim3(kThreads), 0, s, y, (long long)n_docs, N, (long long)N, wt, parts);
        if (int rc = launch_status()) return rc;
        return ltr_enc_sum_partials(parts, grid, N, 0, out, s);
    };
    // dW [M][N] = dz^T h over the documents, both operands k-major, split over the documents
    auto dweight = [&](const float *dz, int M, const float *h, int N, float *out) -> int {
        ltr_gemm_f32_desc d{};
        d.A = dz; d.lda = M; d.a_kmajor = 1;
        d.B = h; d.ldb = N; d.b_kmajor = 1;
        d.M = M; d.N = N; d.K = n_docs; d.ldc = N;
        d.splits = wide_splits(M, N, n_docs, grid);
        d.C = d.splits > 1 ? parts : out;
        if (int rc = gemm(d, s)) return rc;
        return d.splits > 1 ? ltr_enc_sum_partials(parts, d.splits, (long long)M * N, 0, out, s) : LTR_OK;
    };

    // d w3 = sum_d ds_d h_d, d b3 = sum_d ds_d
    if (int rc = colsum(hl, Hl, dscores, gw3)) return rc;
    if (int rc = colsum(dscores, 1, nullptr, gb3)) return rc;
    // dz of the last hidden layer = (ds (x) w3) through the saved activation: the K = 1 form of the GEMM with the gate epilogue
    ltr_gemm_f32_desc d{};
    d.A = dscores; d.lda = 1; d.B = w3; d.ldb = 1;
    d.M = n_docs; d.N = Hl; d.K = 1; d.ldc = Hl; d.splits = 1;
    d.C = dzl;
    d.gate = hl; d.ldg = Hl;
    d.gate_kind = two ? LTR_GEMM_GATE_SIGMOID : LTR_GEMM_GATE_RELU;
    d.gate_scale = slope;
    if (int rc = gemm(d, s)) return rc;
    if (!two) {
        if (int rc = dweight(dzl, H2, acts, H1, gW2)) return rc;
        if (int rc = colsum(dzl, H2, nullptr, gb2)) return rc;
        // dz1 = (dz2 W2) through h1
        d.A = dzl; d.lda = H2; d.B = params[2]; d.ldb = H1; d.b_kmajor = 1;
        d.N = H1; d.K = H2; d.ldc = H1;
        d.C = dz1;
        d.gate = acts; d.ldg = H1;
        if (int rc = gemm(d, s)) return rc;
    }
    if (int rc = dweight(dz1, H1, X, F, gW1)) return rc;
    return colsum(dz1, H1, nullptr, gb1);
}

}  // extern "C"
