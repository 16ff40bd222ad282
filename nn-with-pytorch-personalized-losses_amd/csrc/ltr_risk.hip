// ltr_risk.hip -- risk-sensitive evaluation functions on a [queries x systems] effectiveness matrix (gfx950).
//
// Replaces, behind the reference's Python surface:
//   losses/riskLosses/riskFunctions.py:4-22   zRisk(mat, alpha, requires_grad, i)
//   losses/riskLosses/riskFunctions.py:25-33  geoRisk(mat, alpha, requires_grad, i)
//   losses/riskLosses/riskLosses.py:247-291   the tRisk tail (mean / std of the alpha-weighted deltas)
// The matrix is tiny next to the slate tensors (Q x <= ~10 systems): these are latency-bound reductions, so
// each runs as ONE workgroup that sweeps the matrix three times (column/row sums -> standardised residuals ->
// gradient) with fp64 accumulators and fixed-order cross-wave sums (bit-reproducible).  Forward value and the
// analytic gradient w.r.t. every matrix entry come out of the same launch.
#include "../../include/ltr_mi355x.h"
#include "ltr_device.h"
#include <math.h>

using namespace ltr;

namespace {

constexpr int kRiskThreads = 1024;

__device__ __forceinline__ double wave_allsum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, LTR_WAVE);
    return v;   // butterfly: every lane holds the same bits
}

// sum over the block; every thread gets the total (fixed order: lanes by butterfly, waves sequentially)
__device__ __forceinline__ double block_sum_f64(double v, double *red) {
    v = wave_allsum_f64(v);
    __syncthreads();
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0) red[threadIdx.x / LTR_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kRiskThreads / LTR_WAVE; ++w) s += red[w];
    return s;
}

// zRisk:  si = sum_q mat[q,i];  t_q = sum_j mat[q,j];  n = sum_q t_q;  e_q = si t_q / n;
//         d_q = (mat[q,i] - e_q) / sqrt(e_q);  Z = sum_q d_q (1 + alpha [d_q < 0])                 (:5-22)
// geoRisk: sqrt((si / Q) * Phi(Z / Q)), Phi = standard normal cdf                                   (:26-33)
// dmat (optional): d value / d mat[q,j] (closed form; the indicator [d_q < 0] carries no gradient, like the
// reference's boolean mask).
__global__ void __launch_bounds__(kRiskThreads)
risk_kernel(const float *__restrict__ mat, int Q, int n, int col, float alpha, int geo, int guard,
            float *__restrict__ value, float *__restrict__ dmat) {
    __shared__ double red[kRiskThreads / LTR_WAVE];
    const int tid = threadIdx.x;
    double s_i = 0.0, s_n = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const float *row = mat + (size_t)q * n;
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += (double)row[j];
        s_n += t;
        s_i += (double)row[col];
    }
    const double si = block_sum_f64(s_i, red);
    const double nn = block_sum_f64(s_n, red);
    double z_acc = 0.0, t1_acc = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const float *row = mat + (size_t)q * n;
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += (double)row[j];
        const double x = (double)row[col];
        const double e = si * (t / nn);
        const bool dead = guard && e == 0.0;                       // numpy metric: e == 0 contributes 0 (metrics.py:30-33)
        const double d = dead ? 0.0 : (x - e) / sqrt(e);
        const double c = (guard ? (x - e < 0.0) : (d < 0.0)) ? 1.0 + (double)alpha : 1.0;
        z_acc += c * d;
        const double A = dead ? 0.0 : c * (-0.5 * (x + e) / (e * sqrt(e)));     // c_q * d d_q / d e_q
        t1_acc += A * t;
    }
    const double Z = block_sum_f64(z_acc, red);
    const double T1 = block_sum_f64(t1_acc, red) / nn;              // sum_r A_r t_r / n
    double val = Z, dZ = 1.0, dSi = 0.0;
    if (geo) {
        const double v = Z / (double)Q;
        const double Phi = 0.5 * erfc(-v * 0.70710678118654752440);
        const double phi = 0.39894228040143267794 * exp(-0.5 * v * v);
        const double M = si / (double)Q;
        val = sqrt(M * Phi);
        dZ = 0.5 / val * M * phi / (double)Q;
        dSi = 0.5 / val * Phi / (double)Q;
    }
    if (tid == 0) value[0] = (float)val;
    if (!dmat) return;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const float *row = mat + (size_t)q * n;
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += (double)row[j];
        const double x = (double)row[col];
        const double e = si * (t / nn);
        const bool dead = guard && e == 0.0;
        const double rs = dead ? 0.0 : 1.0 / sqrt(e);
        const double d = (x - e) * rs;
        const double c = (guard ? (x - e < 0.0) : (d < 0.0)) ? 1.0 + (double)alpha : 1.0;
        const double A = dead ? 0.0 : c * (-0.5 * (x + e) * rs / e);
        const double common = A * si / nn - si * T1 / nn;          // via t_q and via n
        const double own = c * rs + T1;                             // via mat[q,i] itself and via si
        for (int j = 0; j < n; ++j) {
            double gz = common + (j == col ? own : 0.0);
            dmat[(size_t)q * n + j] = (float)(dZ * gz + (j == col ? dSi : 0.0));
        }
    }
}

// tRisk tail: delta_q = (a_q - b_q)(1 + alpha [a_q < b_q]);  value = mean(delta) / std(delta)  (unbiased std)
// da / db (optional): d value / d a_q, d value / d b_q.                       riskLosses.py:278-291 / :332-345
__global__ void __launch_bounds__(kRiskThreads)
trisk_kernel(const float *__restrict__ a, const float *__restrict__ b, int Q, float alpha, float *__restrict__ value,
             float *__restrict__ da, float *__restrict__ db) {
    __shared__ double red[kRiskThreads / LTR_WAVE];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const double x = (double)a[q] - (double)b[q];
        s += x * (a[q] < b[q] ? 1.0 + (double)alpha : 1.0);
    }
    const double mu = block_sum_f64(s, red) / (double)Q;
    double v = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const double x = ((double)a[q] - (double)b[q]) * (a[q] < b[q] ? 1.0 + (double)alpha : 1.0);
        v += (x - mu) * (x - mu);
    }
    const double var = block_sum_f64(v, red) / (double)(Q - 1);
    const double se = sqrt(var);
    if (tid == 0) value[0] = (float)(mu / se);
    if (!da && !db) return;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const double c = a[q] < b[q] ? 1.0 + (double)alpha : 1.0;
        const double x = ((double)a[q] - (double)b[q]) * c;
        const double g = (1.0 / ((double)Q * se) - mu * (x - mu) / ((double)(Q - 1) * se * var)) * c;
        if (da) da[q] = (float)g;
        if (db) db[q] = (float)(-g);
    }
}

// Row maps of the two tails.  A dense matrix is ONE block of Q rows.  The data-parallel risk step (ltr_mi355x.scorer.FusedRanker under
// ltr_mi355x.dp.QueryShardedTrainer) hands the tails the all-gathered per-rank blocks instead: block k = one float holding its row
// count, then `block_rows` rows of n floats (a rank's rows, padded to the largest shard).  Logical row q runs over the valid rows only,
// in block order, so a padded gather is summed in exactly the order of the dense matrix it stands for.  The counts are read on the
// device: no host round trip for ragged shards.
constexpr int kMaxRowBlocks = 1024;
struct RowBlocks {
    const int *pre;     // LDS [n_blocks + 1]: prefix sums of the block row counts
    int n_blocks, stride, hdr, n, Q;
    __device__ __forceinline__ size_t row(int q) const {     // offset of logical row q's first element
        int lo = 0, hi = n_blocks - 1;
        while (lo < hi) {                                     // the last block k with pre[k] <= q
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= q) lo = mid; else hi = mid - 1;
        }
        return (size_t)lo * stride + hdr + (size_t)(q - pre[lo]) * n;
    }
};
// all threads call it (one barrier inside)
__device__ __forceinline__ RowBlocks row_blocks(int n_blocks, int block_rows, int n, int hdr, const float *base, int *pre) {
    RowBlocks rb;
    rb.stride = hdr + block_rows * n;
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int k = 0; k < n_blocks; ++k) {
            pre[k] = acc;
            int c = hdr ? (int)base[(size_t)k * rb.stride] : block_rows;
            acc += c < 0 ? 0 : (c > block_rows ? block_rows : c);
        }
        pre[n_blocks] = acc;
    }
    __syncthreads();
    rb.pre = pre;
    rb.n_blocks = n_blocks;
    rb.hdr = hdr;
    rb.n = n;
    rb.Q = pre[n_blocks];
    return rb;
}

// The TAIL of a tRisk loss in one launch (riskLosses.py:269-291 / :332-345) on the [Q][2] matrix (model, baseline): the flip of
// transformation 1 (mat' = -mat + max(mat), exact in fp64), the alpha-weighted deltas, mean / std, the
// `negative` factor; value and d value / d mat together.  The flip's whole-matrix maximum gets no gradient: the gradients of the
// two columns of a query are g and -g, so their sum over the matrix is zero.
__global__ void __launch_bounds__(kRiskThreads)
trisk_tail_kernel(const float *__restrict__ mat, int n_blocks, int block_rows, int hdr, float alpha, int flip, float factor,
                  float *__restrict__ value, float *__restrict__ dmat) {
    __shared__ double red[kRiskThreads / LTR_WAVE];
    __shared__ int pre[kMaxRowBlocks + 1];
    const int tid = threadIdx.x;
    const RowBlocks rb = row_blocks(n_blocks, block_rows, 2, hdr, mat, pre);
    const int Q = rb.Q;
    float M = 0.f;
    if (flip) {
        float mx = -INFINITY;
        for (int e = tid; e < 2 * Q; e += kRiskThreads) mx = fmaxf(mx, mat[rb.row(e >> 1) + (e & 1)]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, LTR_WAVE));
        __syncthreads();
        if ((tid & (LTR_WAVE - 1)) == 0) red[tid / LTR_WAVE] = (double)mx;
        __syncthreads();
        M = (float)red[0];
        for (int w = 1; w < kRiskThreads / LTR_WAVE; ++w) M = fmaxf(M, (float)red[w]);
        __syncthreads();
    }
    auto at = [&](int q, int j) -> double { const double x = (double)mat[rb.row(q) + j]; return flip ? (double)M - x : x; };   // exact
    double s = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const double a = at(q, 0), b = at(q, 1);
        s += (a - b) * (a < b ? 1.0 + (double)alpha : 1.0);
    }
    const double mu = block_sum_f64(s, red) / (double)Q;
    double v = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const double a = at(q, 0), b = at(q, 1);
        const double x = (a - b) * (a < b ? 1.0 + (double)alpha : 1.0);
        v += (x - mu) * (x - mu);
    }
    const double var = block_sum_f64(v, red) / (double)(Q - 1);
    const double se = sqrt(var);
    if (tid == 0) value[0] = (float)(mu / se) * factor;
    if (!dmat) return;
    for (int q = tid; q < Q; q += kRiskThreads) {
        const double a = at(q, 0), b = at(q, 1);
        const double c = a < b ? 1.0 + (double)alpha : 1.0;
        const double x = (a - b) * c;
        const float g = (float)((1.0 / ((double)Q * se) - mu * (x - mu) / ((double)(Q - 1) * se * var)) * c) * factor;
        const size_t r = rb.row(q);
        dmat[r] = flip ? -g : g;
        dmat[r + 1] = flip ? g : -g;
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// The TAIL of a geoRisk / zRisk loss in one launch (riskLosses.py:47-60, :118-125, :170-180, :237-244): the "larger = better" flip
// mat' = -mat + max(mat), the risk of column 0 and (return strategies 2 / 3) of the last column, the strategy's combination, the
// `negative` factor -- value and d value / d mat (w.r.t. the UNFLIPPED matrix; the whole-matrix max passes its gradient to the
// maximal entries, evenly among ties, like torch.max) come out together.
//   strategy 1: f R0      2: f (R1 - R0)   [zquirk: f R1 - R0, the reference's operator precedence in zRiskListnetLoss, :176]
//   strategy 3: f (R1 - R0)^2
struct RiskCol { double si, Z, T1, val, dZ, dSi; };

__global__ void __launch_bounds__(kRiskThreads)
risk_tail_kernel(const float *__restrict__ mat, int n_blocks, int block_rows, int hdr, int n, float alpha, int geo, int strategy, int flip, float factor, int zquirk,
                 float *__restrict__ value, float *__restrict__ dmat) {
    __shared__ double red[kRiskThreads / LTR_WAVE];
    __shared__ int pre[kMaxRowBlocks + 1];
    const int tid = threadIdx.x;
    const RowBlocks rb = row_blocks(n_blocks, block_rows, n, hdr, mat, pre);
    const int Q = rb.Q;
    auto elem = [&](int e) -> size_t { const int q = e / n; return rb.row(q) + (e - q * n); };   // element e of the dense matrix
    double M = 0.0;
    if (flip) {
        double mx = -INFINITY;
        for (int e = tid; e < Q * n; e += kRiskThreads) mx = fmax(mx, (double)mat[elem(e)]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, LTR_WAVE));
        __syncthreads();
        if ((tid & (LTR_WAVE - 1)) == 0) red[tid / LTR_WAVE] = mx;
        __syncthreads();
        M = red[0];
        for (int w = 1; w < kRiskThreads / LTR_WAVE; ++w) M = fmax(M, red[w]);
        M = (double)(float)M;
    }
    // the flipped entry -mat + max, exact in fp64 (both operands are fp32 numbers).  Rounding it to fp32 first, as the reference's
    // tensors do, moved zRisk at alpha = 0 (a cancelling sum of residuals) by 5.8e-5 on a 3 x 9 matrix: tests/test_risk_tails_gpu.py
    auto at = [&](int q, int j) -> double { const double x = (double)mat[rb.row(q) + j]; return flip ? M - x : x; };
    const int ncol = strategy == 1 ? 1 : 2;
    const int cols[2] = {0, n - 1};
    RiskCol rc[2];
    double s_n = 0.0, s_i0 = 0.0, s_i1 = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += at(q, j);
        s_n += t;
        s_i0 += at(q, 0);
        s_i1 += at(q, n - 1);
    }
    const double nn = block_sum_f64(s_n, red);
    rc[0].si = block_sum_f64(s_i0, red);
    rc[1].si = block_sum_f64(s_i1, red);
    for (int i = 0; i < ncol; ++i) {
        const double si = rc[i].si;
        double z_acc = 0.0, t1_acc = 0.0;
        for (int q = tid; q < Q; q += kRiskThreads) {
            double t = 0.0;
            for (int j = 0; j < n; ++j) t += at(q, j);
            const double x = at(q, cols[i]);
            const double e = si * (t / nn);
            const double d = (x - e) / sqrt(e);
            const double c = d < 0.0 ? 1.0 + (double)alpha : 1.0;
            z_acc += c * d;
            t1_acc += c * (-0.5 * (x + e) / (e * sqrt(e))) * t;
        }
        rc[i].Z = block_sum_f64(z_acc, red);
        rc[i].T1 = block_sum_f64(t1_acc, red) / nn;
        rc[i].val = rc[i].Z;
        rc[i].dZ = 1.0;
        rc[i].dSi = 0.0;
        if (geo) {
            const double v = rc[i].Z / (double)Q;
            const double Phi = 0.5 * erfc(-v * 0.70710678118654752440);
            const double phi = 0.39894228040143267794 * exp(-0.5 * v * v);
            const double Mq = si / (double)Q;
            rc[i].val = sqrt(Mq * Phi);
            rc[i].dZ = 0.5 / rc[i].val * Mq * phi / (double)Q;
            rc[i].dSi = 0.5 / rc[i].val * Phi / (double)Q;
        }
    }
    // the reference evaluates each risk in fp32 tensors: round the two values where it does before combining them
    const double R0 = (double)(float)rc[0].val, R1 = ncol > 1 ? (double)(float)rc[1].val : 0.0, f = (double)factor;
    double out, c0, c1 = 0.0;
    if (strategy == 1) { out = f * R0; c0 = f; }
    else if (strategy == 2) {
        if (zquirk) { out = f * R1 - R0; c0 = -1.0; c1 = f; }
        else { out = f * (R1 - R0); c0 = -f; c1 = f; }
    } else { const double df = R1 - R0; out = f * df * df; c0 = -2.0 * f * df; c1 = 2.0 * f * df; }
    if (tid == 0) value[0] = (float)out;
    if (!dmat) return;
    const double coef[2] = {c0, c1};
    double g_acc = 0.0;
    for (int q = tid; q < Q; q += kRiskThreads) {
        double t = 0.0;
        for (int j = 0; j < n; ++j) t += at(q, j);
        double common = 0.0, own[2] = {0.0, 0.0};
        for (int i = 0; i < ncol; ++i) {
            const double si = rc[i].si, x = at(q, cols[i]);
            const double e = si * (t / nn), rs = 1.0 / sqrt(e), d = (x - e) * rs;
            const double c = d < 0.0 ? 1.0 + (double)alpha : 1.0;
            const double A = c * (-0.5 * (x + e) * rs / e);
            common += coef[i] * rc[i].dZ * (A * si / nn - si * rc[i].T1 / nn);
            own[i] = coef[i] * (rc[i].dZ * (c * rs + rc[i].T1) + rc[i].dSi);
        }
        for (int j = 0; j < n; ++j) {
            double gq = common;
            if (j == 0) gq += own[0];
            if (ncol > 1 && j == n - 1) gq += own[1];
            g_acc += gq;
            dmat[rb.row(q) + j] = (float)(flip ? -gq : gq);
        }
    }
    if (flip) {      // d max(mat) / d mat: the sum of all d value / d mat' entries lands on the maximal entries
        const double G = block_sum_f64(g_acc, red);
        double ties_a = 0.0;
        for (int e = tid; e < Q * n; e += kRiskThreads) ties_a += (double)mat[elem(e)] == M ? 1.0 : 0.0;
        const double ties = block_sum_f64(ties_a, red);
        for (int e = tid; e < Q * n; e += kRiskThreads)
            if ((double)mat[elem(e)] == M) dmat[elem(e)] += (float)(G / ties);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The [queries x systems] effectiveness matrix of the risk-sensitive losses, one workgroup per query, one launch for all systems
// (riskLosses.py:8-49 / :128-169 / :247-276 Listnet type, :63-117 / :183-236 / :294-330 Lambda type) -- and d mat[q][0] / d (the
// model's input), the only gradient the losses need (column 0 is the model; baselines and the ideal ranking are constants).
//   mode 0 (Listnet type): ref = labels, x0 = the model's scores, rest = baseline scores [B][S][nr]; every vector is soft-maxed over
//     the slate first (:10-12);  lt 1: sum_j (t p - t^2)^2   lt 2: cos(t, p)   lt 3: (sum t p - sum t^2)^2        (:16-46)
//   mode 1 (Lambda type): ref / x0 / rest [nr][B][S] are the lambdaMask column sums, used as they are;
//     lt 1: sum_j (x - t)^2   lt 2: cos(t, x)   lt 3: (sum x - sum t)^2                                          (:71-104)
//   mode 2 (the tRisk Listnet loss, :247-276): as mode 0, but transformation 2 is the cosine of the PRODUCTS, cos(t^2, t p).
//   ideal != 0 appends the column of the reference vector itself.
// fp32 elementwise arithmetic, fp64 sums, fixed-order reductions.  The cosine follows ATen: w12 / sqrt(max(w1 w2, eps^2)), eps 1e-8.
constexpr int kMatThreads = 256;
constexpr int kMatMaxS = 2048;

__device__ __forceinline__ double mat_block_sum(double v, double *red) {
    v = wave_allsum_f64(v);
    __syncthreads();
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0) red[threadIdx.x / LTR_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kMatThreads / LTR_WAVE; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ float mat_block_max(float v, double *red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, LTR_WAVE));
    __syncthreads();
    if ((threadIdx.x & (LTR_WAVE - 1)) == 0) red[threadIdx.x / LTR_WAVE] = (double)v;
    __syncthreads();
    float m = -INFINITY;
    for (int w = 0; w < kMatThreads / LTR_WAVE; ++w) m = fmaxf(m, (float)red[w]);
    return m;
}
// in place: v[0..S) -> softmax(v) (torch: exp(x - max) / sum)
__device__ __forceinline__ void mat_softmax(float *v, int S, double *red) {
    float m = -INFINITY;
    for (int j = threadIdx.x; j < S; j += kMatThreads) m = fmaxf(m, v[j]);
    m = mat_block_max(m, red);
    double z = 0.0;
    for (int j = threadIdx.x; j < S; j += kMatThreads) {
        const float e = expf(v[j] - m);
        v[j] = e;
        z += (double)e;
    }
    const float inv = (float)(1.0 / mat_block_sum(z, red));
    for (int j = threadIdx.x; j < S; j += kMatThreads) v[j] *= inv;
    __syncthreads();
}

// One query's row: b = its row of mat / cached, off = its first document row, S = its length.  Mode 1 keeps system k's column sums at
// rest[(k - 1) * sys_stride + off ..] (sys_stride = the documents of the whole batch).  Shared by the rectangular kernel (off = b S) and
// the ragged one: same threads, same strides, same bits.
__device__ __forceinline__ void risk_matrix_row(const float *__restrict__ ref, const float *__restrict__ x0, const float *__restrict__ rest,
                                                const size_t b, const size_t off, const int S, const size_t sys_stride, int nr, int mode,
                                                int lt, int ideal, int ones, const float *__restrict__ cached, int cache_stride,
                                                float *__restrict__ mat, float *__restrict__ jac, float *smem, double *red) {
    float *t = smem, *x = smem + S;
    // cached != NULL: columns 1 .. nr come from cached[b][0 .. nr) (the constant systems, ltr_risk_matrix_cached_fwd); only the model runs
    // ones != 0: one more column of 1.0 after the computed ones (geoRiskLambdaLoss's ideal ranking under transformation 2, :106)
    const int tid = threadIdx.x, nsys = 1 + nr + (ideal && !cached ? 1 : 0), nrun = cached ? 1 : nsys;
    const int ld = nsys + (ones && !cached ? 1 : 0);
    if (cached)
        for (int k = tid; k < nr; k += kMatThreads) mat[b * ld + 1 + k] = cached[b * cache_stride + k];
    if (ld > nsys && tid == 0) mat[b * ld + nsys] = 1.0f;
    for (int j = tid; j < S; j += kMatThreads) t[j] = ref[off + j];
    __syncthreads();
    if (mode != 1) mat_softmax(t, S, red);
    double nt_a = 0.0, st_a = 0.0;
    for (int j = tid; j < S; j += kMatThreads) {
        nt_a += (double)t[j] * t[j];
        st_a += (double)t[j];
    }
    const double nt = mat_block_sum(nt_a, red), st = mat_block_sum(st_a, red);
    for (int sys = 0; sys < nrun; ++sys) {
        const bool is_ideal = ideal && !cached && sys == nsys - 1;
        __syncthreads();
        for (int j = tid; j < S; j += kMatThreads) {
            float v;
            if (is_ideal) v = t[j];
            else if (sys == 0) v = x0[off + j];
            else v = mode != 1 ? rest[(off + j) * nr + (sys - 1)] : rest[(size_t)(sys - 1) * sys_stride + off + j];
            x[j] = v;
        }
        __syncthreads();
        if (mode != 1 && !is_ideal) mat_softmax(x, S, red);
        double a_a = 0.0, nx_a = 0.0, c_a = 0.0, sx_a = 0.0, ac_a = 0.0, nu_a = 0.0, nv_a = 0.0;
        for (int j = tid; j < S; j += kMatThreads) {
            const float tj = t[j], xj = x[j];
            a_a += (double)tj * xj;
            nx_a += (double)xj * xj;
            sx_a += (double)xj;
            const float df = mode == 1 ? xj - tj : tj * xj - tj * tj;
            c_a += (double)df * df;
            if (mode == 2) {                       // the tRisk pair's cosine is taken between the PRODUCTS t^2 and t x (:256-258)
                const float u = tj * tj, v = tj * xj;
                ac_a += (double)u * v;
                nu_a += (double)u * u;
                nv_a += (double)v * v;
            }
        }
        const double a = mat_block_sum(a_a, red), nx = mat_block_sum(nx_a, red), c = mat_block_sum(c_a, red), sx = mat_block_sum(sx_a, red);
        // cosine operands: (u, v) = (t, x) [modes 0, 1] or (t^2, t x) [mode 2]
        const double ca = mode == 2 ? mat_block_sum(ac_a, red) : a, cnu = mode == 2 ? mat_block_sum(nu_a, red) : nt,
                     cnv = mode == 2 ? mat_block_sum(nv_a, red) : nx;
        // torch.nn.CosineSimilarity (riskLosses.py: nn.CosineSimilarity(dim=1), eps = 1e-8) clamps EACH norm: u . v / (max(|u|, eps) max(|v|, eps))
        const double nrm_u = sqrt(cnu), nrm_v = sqrt(cnv);
        const double den = (nrm_u > 1e-8 ? nrm_u : 1e-8) * (nrm_v > 1e-8 ? nrm_v : 1e-8);
        double m;
        if (lt == 1) m = c;
        else if (lt == 2) m = ca / den;
        else m = mode == 1 ? (sx - st) * (sx - st) : (a - nt) * (a - nt);
        if (tid == 0) mat[b * ld + sys] = (float)m;
        if (sys == 0 && jac) {
            // g_j = d m / d x_j; mode 0: x = softmax(s): d m / d s_j = x_j (g_j - sum_k x_k g_k)
            // The installed torch (2.10, ATen cosine_similarity) clamps the two norms IN PLACE under no-grad: the VALUE uses
            // max(|v|, eps), the gradient still flows through the norm as d|v| / dv = v / |v| (0 at v = 0) -- measured on a vector of
            // norm 3e-9 (tests/test_risk_gpu.py::test_fused_risk_matrix_cosine_of_a_zero_vector):
            //   d m / d v = u / den - m v / (max(|v|, eps) |v|)
            const double nv_c = nrm_v > 1e-8 ? nrm_v : 1e-8;
            const double inv_vv = nrm_v > 0.0 ? 1.0 / (nv_c * nrm_v) : 0.0;
            auto grad = [&](int j) -> double {
                const double tj = t[j], xj = x[j];
                if (lt == 1) return mode == 1 ? 2.0 * (xj - tj) : 2.0 * tj * (tj * xj - tj * tj);
                if (lt == 2) {
                    const double u = mode == 2 ? tj * tj : tj, v = mode == 2 ? tj * xj : xj, w = mode == 2 ? tj : 1.0;
                    return w * (u / den - m * v * inv_vv);
                }
                return mode == 1 ? 2.0 * (sx - st) : 2.0 * (a - nt) * tj;
            };
            if (mode != 1) {
                double dot_a = 0.0;
                for (int j = tid; j < S; j += kMatThreads) dot_a += (double)x[j] * grad(j);
                const double dot = mat_block_sum(dot_a, red);
                for (int j = tid; j < S; j += kMatThreads) jac[off + j] = (float)((double)x[j] * (grad(j) - dot));
            } else {
                for (int j = tid; j < S; j += kMatThreads) jac[off + j] = (float)grad(j);
            }
        }
    }
}

__global__ void __launch_bounds__(kMatThreads)
risk_matrix_kernel(const float *__restrict__ ref, const float *__restrict__ x0, const float *__restrict__ rest, int B, int S, int nr,
                   int mode, int lt, int ideal, int ones, const float *__restrict__ cached, int cache_stride, float *__restrict__ mat,
                   float *__restrict__ jac) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kMatThreads / LTR_WAVE];
    const size_t b = blockIdx.x;
    risk_matrix_row(ref, x0, rest, b, b * S, S, (size_t)B * S, nr, mode, lt, ideal, ones, cached, cache_stride, mat, jac, smem, red);
}

// The ragged batch: query q owns document rows offsets[q] .. offsets[q + 1] - 1, any lengths 1 .. s_max in ONE
// launch -- the kernel runs 256 threads per query whatever its length, so there is no tier here.  The query id, its offset and its
// length are wave-uniform and taken through v_readfirstlane: S and everything derived from it stay in scalar registers, as with the
// rectangular kernel's argument.  A listed query with a length outside 1 .. s_max (the LDS is sized for s_max; the host layer never
// lists one) gets a NaN model entry; none of its rows is read or written.
struct MatQuery {
    long long q, off, len;     // query id, first document row, documents
    bool listed, fits;         // slot < n_queries; 1 <= len <= s_max and its rows inside the batch
};
// (no tier rule here, unlike ltr_losses.hip's ragged_slot: these kernels run the same threads for any length)
__device__ __forceinline__ MatQuery mat_query(const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries,
                                              int s_max, long long n_docs) {
    MatQuery r = {0, 0, 0, false, false};
    const long long slot = ltr_wave_uniform(ltr_block_id());
    if (slot >= n_queries) return r;
    r.listed = true;
    r.q = ltr_wave_uniform(queries ? (long long)queries[slot] : slot);
    r.off = ltr_wave_uniform(offsets[r.q]);
    r.len = ltr_wave_uniform(offsets[r.q + 1]) - r.off;
    r.fits = r.len >= 1 && r.len <= s_max && r.off >= 0 && r.off + r.len <= n_docs;
    return r;
}

__global__ void __launch_bounds__(kMatThreads)
risk_matrix_ragged_kernel(const float *__restrict__ ref, const float *__restrict__ x0, const float *__restrict__ rest,
                          const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, int s_max,
                          long long n_docs, int nr, int mode, int lt, int ideal, int ones, const float *__restrict__ cached,
                          int cache_stride, float *__restrict__ mat, float *__restrict__ jac) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ double red[kMatThreads / LTR_WAVE];
    const MatQuery mq = mat_query(offsets, queries, n_queries, s_max, n_docs);
    if (!mq.listed) return;                      // (whole block: the y-padding of a two-dimensional grid)
    if (!mq.fits) {                              // (whole block)
        const int ld = 1 + nr + (ideal && !cached ? 1 : 0) + (ones && !cached ? 1 : 0);
        if (threadIdx.x == 0) mat[(size_t)mq.q * ld] = NAN;
        return;
    }
    risk_matrix_row(ref, x0, rest, (size_t)mq.q, (size_t)mq.off, (int)mq.len, (size_t)n_docs, nr, mode, lt, ideal, ones, cached,
                    cache_stride, mat, jac, smem, red);
}

// d loss / d x0 of a risk loss whose matrix came from risk_matrix_kernel: ds[b][j] = jac[b][j] * dmat[b][0] (the column-0 entry of
// the tail's gradient, read at a row stride so that a rank's rows of an all-gathered matrix are used in place).
__global__ void __launch_bounds__(256)
risk_scores_grad_kernel(const float *__restrict__ jac, const float *__restrict__ coef, int coef_stride, long long B, int S,
                        float *__restrict__ ds) {
    const long long n = B * (long long)S;
    for (long long e = ltr_block_id() * 256 + threadIdx.x; e < n; e += 256ll * gridDim.x * gridDim.y) {
        const long long b = e / S;
        ds[e] = jac[e] * coef[b * coef_stride];
    }
}

// The same product on a ragged batch: one workgroup per listed query q, ds[d] = jac[d] * coef[q * coef_stride] over q's own rows
// (q, its offset and its length through v_readfirstlane: the coefficient is one scalar load per workgroup).
__global__ void __launch_bounds__(256)
risk_scores_grad_ragged_kernel(const float *__restrict__ jac, const float *__restrict__ coef, int coef_stride,
                               const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, long long n_docs,
                               float *__restrict__ ds) {
    const MatQuery mq = mat_query(offsets, queries, n_queries, kMatMaxS, n_docs);
    if (!mq.listed || !mq.fits) return;          // not a query of a risk batch: its rows stay untouched
    const float c = coef[mq.q * coef_stride];
    for (int j = threadIdx.x; j < (int)mq.len; j += 256) ds[mq.off + j] = jac[mq.off + j] * c;
}

}  // namespace

extern "C" {

int ltr_risk_fwd_bwd(const float *mat, int Q, int n_systems, int col, float alpha, int kind, float *value,
                     float *dmat, void *stream) {
    if (!mat || !value) return LTR_ERR_NULL;
    if (Q < 1 || n_systems < 1 || n_systems > 4096) return LTR_ERR_SHAPE;
    if (col < 0) col += n_systems;                       /* i = -1: the last system, as Python indexes */
    const int guard = (kind & LTR_RISK_ZERO_GUARD) ? 1 : 0;
    kind &= ~LTR_RISK_ZERO_GUARD;
    if (col < 0 || col >= n_systems || (kind != LTR_RISK_Z && kind != LTR_RISK_GEO)) return LTR_ERR_PARAM;
    hipLaunchKernelGGL(risk_kernel, dim3(1), dim3(kRiskThreads), 0, (hipStream_t)stream, mat, Q, n_systems, col, alpha,
                       kind == LTR_RISK_GEO ? 1 : 0, guard, value, dmat);
    return launch_status();
}

int ltr_trisk_fwd_bwd(const float *model, const float *baseline, int Q, float alpha, float *value, float *dmodel,
                      float *dbaseline, void *stream) {
    if (!model || !baseline || !value) return LTR_ERR_NULL;
    if (Q < 1) return LTR_ERR_SHAPE;
    hipLaunchKernelGGL(trisk_kernel, dim3(1), dim3(kRiskThreads), 0, (hipStream_t)stream, model, baseline, Q, alpha, value,
                       dmodel, dbaseline);
    return launch_status();
}

int ltr_trisk_tail_fwd_bwd(const float *mat, int Q, float alpha, int flip, float factor, float *value, float *dmat, void *stream) {
    if (!mat || !value) return LTR_ERR_NULL;
    if (Q < 1 || Q > (1 << 29)) return LTR_ERR_SHAPE;
    hipLaunchKernelGGL(trisk_tail_kernel, dim3(1), dim3(kRiskThreads), 0, (hipStream_t)stream, mat, 1, Q, 0, alpha, flip ? 1 : 0, factor,
                       value, dmat);
    return launch_status();
}

int ltr_risk_tail_fwd_bwd(const float *mat, int Q, int n_systems, float alpha, int kind, int strategy, int flip, float factor,
                          int zquirk, float *value, float *dmat, void *stream) {
    if (!mat || !value) return LTR_ERR_NULL;
    if (Q < 1 || n_systems < 1 || (long long)Q * n_systems > (1ll << 30)) return LTR_ERR_SHAPE;
    if ((kind != 0 && kind != 1) || strategy < 1 || strategy > 3) return LTR_ERR_PARAM;
    hipLaunchKernelGGL(risk_tail_kernel, dim3(1), dim3(kRiskThreads), 0, (hipStream_t)stream, mat, 1, Q, 0, n_systems, alpha, kind, strategy,
                       flip ? 1 : 0, factor, zquirk ? 1 : 0, value, dmat);
    return launch_status();
}

int ltr_risk_tail_blocks_fwd_bwd(const float *blocks, int n_blocks, int block_rows, int n_systems, float alpha, int kind, int strategy,
                                 int flip, float factor, int zquirk, float *value, float *dmat, void *stream) {
    if (!blocks || !value) return LTR_ERR_NULL;
    if (n_blocks < 1 || n_blocks > kMaxRowBlocks || block_rows < 0 || n_systems < 1 ||
        (long long)n_blocks * block_rows * n_systems > (1ll << 30))
        return LTR_ERR_SHAPE;
    if ((kind != 0 && kind != 1) || strategy < 1 || strategy > 3) return LTR_ERR_PARAM;
    hipLaunchKernelGGL(risk_tail_kernel, dim3(1), dim3(kRiskThreads), 0, (hipStream_t)stream, blocks, n_blocks, block_rows, 1, n_systems,
                       alpha, kind, strategy, flip ? 1 : 0, factor, zquirk ? 1 : 0, value, dmat);
    return launch_status();
}

int ltr_trisk_tail_blocks_fwd_bwd(const float *blocks, int n_blocks, int block_rows, float alpha, int flip, float factor, float *value,
                                  float *dmat, void *stream) {
    if (!blocks || !value) return LTR_ERR_NULL;
    if (n_blocks < 1 || n_blocks > kMaxRowBlocks || block_rows < 0 || (long long)n_blocks * block_rows > (1 << 29)) return LTR_ERR_SHAPE;
    hipLaunchKernelGGL(trisk_tail_kernel, dim3(1), dim3(kRiskThreads), 0, (hipStream_t)stream, blocks, n_blocks, block_rows, 1, alpha,
                       flip ? 1 : 0, factor, value, dmat);
    return launch_status();
}

int ltr_risk_matrix_rows_fwd(const float *ref, const float *x0, const float *rest, int B, int S, int n_rest, int mode, int lt, int ideal,
                             int ones, float *mat, float *jac, void *stream) {
    if (!ref || !x0 || !mat || (n_rest > 0 && !rest)) return LTR_ERR_NULL;
    if (B < 0 || S < 1 || S > kMatMaxS || n_rest < 0 || n_rest > 64) return LTR_ERR_SHAPE;
    if (mode < 0 || mode > 2 || lt < 1 || lt > 3) return LTR_ERR_PARAM;
    if (B == 0) return LTR_OK;
    hipLaunchKernelGGL(risk_matrix_kernel, dim3(B), dim3(kMatThreads), (size_t)2 * S * sizeof(float), (hipStream_t)stream, ref, x0, rest, B,
                       S, n_rest, mode, lt, ideal ? 1 : 0, ones ? 1 : 0, nullptr, 0, mat, jac);
    return launch_status();
}

int ltr_risk_matrix_cached_fwd(const float *ref, const float *x0, const float *cached, int cache_stride, int B, int S, int n_cached,
                               int mode, int lt, float *mat, float *jac, void *stream) {
    if (!ref || !x0 || !mat || (n_cached > 0 && !cached)) return LTR_ERR_NULL;
    if (B < 0 || S < 1 || S > kMatMaxS || n_cached < 0 || n_cached > 65 || cache_stride < n_cached) return LTR_ERR_SHAPE;
    if (mode < 0 || mode > 2 || lt < 1 || lt > 3) return LTR_ERR_PARAM;
    if (B == 0) return LTR_OK;
    hipLaunchKernelGGL(risk_matrix_kernel, dim3(B), dim3(kMatThreads), (size_t)2 * S * sizeof(float), (hipStream_t)stream, ref, x0,
                       cached ? cached : x0, B, S, n_cached, mode, lt, 0, 0, cached ? cached : x0, cache_stride, mat, jac);
    return launch_status();
}

int ltr_risk_scores_grad(const float *jac, const float *dmat, int dmat_stride, int B, int S, float *dscores, void *stream) {
    if (!jac || !dmat || !dscores) return LTR_ERR_NULL;
    if (B < 0 || S < 1 || dmat_stride < 1) return LTR_ERR_SHAPE;
    if (B == 0) return LTR_OK;
    const long long blocks = ((long long)B * S + 255) / 256;
    hipLaunchKernelGGL(risk_scores_grad_kernel, ltr_grid(blocks < 4096 ? blocks : 4096), dim3(256), 0, (hipStream_t)stream, jac, dmat,
                       dmat_stride, (long long)B, S, dscores);
    return launch_status();
}

int ltr_risk_matrix_fwd(const float *ref, const float *x0, const float *rest, int B, int S, int n_rest, int mode, int lt, int ideal,
                        float *mat, float *jac, void *stream) {
    if (!ref || !x0 || !mat || (n_rest > 0 && !rest)) return LTR_ERR_NULL;
    if (B < 0 || S < 1 || S > kMatMaxS || n_rest < 0 || n_rest > 64) return LTR_ERR_SHAPE;
    if (mode < 0 || mode > 2 || lt < 1 || lt > 3) return LTR_ERR_PARAM;
    if (B == 0) return LTR_OK;
    hipLaunchKernelGGL(risk_matrix_kernel, dim3(B), dim3(kMatThreads), (size_t)2 * S * sizeof(float), (hipStream_t)stream, ref, x0, rest, B,
                       S, n_rest, mode, lt, ideal ? 1 : 0, 0, nullptr, 0, mat, jac);
    return launch_status();
}

int ltr_risk_matrix_ragged_fwd(const float *ref, const float *x0, const float *rest, const int64_t *offsets, const int32_t *queries,
                               int n_queries, int s_max, int64_t n_docs, int n_rest, int mode, int lt, int ideal, int ones,
                               const float *cached, int cache_stride, float *mat, float *jac, void *stream) {
    if (!ref || !x0 || !mat || !offsets || (n_rest > 0 && !rest && !cached)) return LTR_ERR_NULL;
    if (n_queries < 0 || s_max < 1 || s_max > kMatMaxS || n_docs < 0 || n_rest < 0 || n_rest > (cached ? 65 : 64)) return LTR_ERR_SHAPE;
    if (cached && (cache_stride < n_rest || ideal || ones)) return LTR_ERR_SHAPE;
    if (mode < 0 || mode > 2 || lt < 1 || lt > 3) return LTR_ERR_PARAM;
    if (n_queries == 0) return LTR_OK;
    hipLaunchKernelGGL(risk_matrix_ragged_kernel, ltr_grid(n_queries), dim3(kMatThreads), (size_t)2 * s_max * sizeof(float),
                       (hipStream_t)stream, ref, x0, cached ? cached : rest, offsets, queries, n_queries, s_max, (long long)n_docs, n_rest,
                       mode, lt, ideal ? 1 : 0, ones ? 1 : 0, cached, cache_stride, mat, jac);
    return launch_status();
}

int ltr_risk_scores_grad_ragged(const float *jac, const float *dmat, int dmat_stride, const int64_t *offsets, const int32_t *queries,
                                int n_queries, int64_t n_docs, float *dscores, void *stream) {
    if (!jac || !dmat || !dscores || !offsets) return LTR_ERR_NULL;
    if (n_queries < 0 || n_docs < 0 || dmat_stride < 1) return LTR_ERR_SHAPE;
    if (n_queries == 0) return LTR_OK;
    hipLaunchKernelGGL(risk_scores_grad_ragged_kernel, ltr_grid(n_queries), dim3(256), 0, (hipStream_t)stream, jac, dmat, dmat_stride,
                       offsets, queries, n_queries, (long long)n_docs, dscores);
    return launch_status();
}

}  // extern "C"
