/*
 * ltr_mi355x.h -- C ABI of libltr_mi355x.so: the MI355X (gfx950) listwise learning-to-rank hot path.
 *
 * The reference (Haiga/nn-with-pytorch-personalized-losses) has no FFI layer: its boundary for this path
 * is the Python import surface.  Every entry point below therefore replaces one
 * reference *Python function* (file:line given per entry); the Python host code under
 * nn-with-pytorch-personalized-losses_amd/{losses,architeture}/ keeps the reference's names/signatures and
 * binds these symbols through ctypes (see INTEGRATION.md for the binding stub).
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM) unless marked host.  Row-major, contiguous, fp32 unless noted.
 *   - `stream` is a hipStream_t passed as void*.  Launchers never allocate, never synchronise, never throw.
 *   - Return value: 0 = launched; < 0 = argument rejected before any launch (LTR_ERR_*); > 0 = hipError_t.
 *   - "slate" = one query's documents; B slates of S documents each; F features per document.
 *   - Per-slate partial results are written; the final mean/sum over slates is a deterministic
 *     fixed-order reduction (ltr_reduce_sum_f32), never a float atomic.
 */
#ifndef LTR_MI355X_H
#define LTR_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTR_ABI_VERSION 1

enum {
    LTR_OK = 0,
    LTR_ERR_NULL = -1,   /* required pointer is NULL                      */
    LTR_ERR_SHAPE = -2,  /* B/S/F/n outside what the kernels support       */
    LTR_ERR_PARAM = -3,  /* bad enum / scalar (scheme id, log base, ...)   */
    LTR_ERR_ALIGN = -4,  /* pointer not aligned as the entry point states  */
    LTR_ERR_IO = -5,     /* (host entry points) file cannot be opened/mapped */
    LTR_ERR_PARSE = -6   /* (host entry points) malformed input line        */
};

/* Largest slate length the loss kernels take (LDS-resident slate state). */
#define LTR_MAX_SLATE 2048

/* lambdaLoss weighing schemes, losses/lambdaL.py:96-127 (string-dispatched there, :46). */
enum {
    LTR_SCHEME_NONE = 0,                 /* weighing_scheme=None                      -> w = 1              */
    LTR_SCHEME_NDCG_LOSS1 = 1,           /* ndcgLoss1_scheme                  :96-97                        */
    LTR_SCHEME_NDCG_LOSS2 = 2,           /* ndcgLoss2_scheme                  :100-106                      */
    LTR_SCHEME_LAMBDA_RANK = 3,          /* lamdbaRank_scheme [sic]           :109-111                      */
    LTR_SCHEME_NDCG_LOSS2PP = 4,         /* ndcgLoss2PP_scheme                :114-115                      */
    LTR_SCHEME_RANKNET = 5,              /* rankNet_scheme                    :118-119                      */
    LTR_SCHEME_RANKNET_GT_DIFF = 6,      /* rankNetWeightedByGTDiff_scheme    :122-123                      */
    LTR_SCHEME_RANKNET_GT_DIFF_POW = 7   /* rankNetWeightedByGTDiffPowed_scheme :126-127                    */
};
enum { LTR_LOG_BINARY = 0, LTR_LOG_NATURAL = 1 }; /* reduction_log, lambdaL.py:52-57 */

int ltr_abi_version(void);
/* Static description of a return code (LTR_ERR_* or hipError_t). Host pointer, never NULL. */
const char *ltr_error_string(int code);

/* out[0] = scale * sum(in[0..n)), fixed summation order (bit-reproducible). */
int ltr_reduce_sum_f32(const float *in, int64_t n, float scale, float *out, void *stream);

/* ---- approxNDCGLoss(y_pred, y_true, eps, padded_value_indicator, alpha)   losses/approxNDCG.py:7-53
 * One pass, one workgroup-slice per slate: soft ranks from pairwise sigmoids in LDS, forward and
 * analytic backward together.
 *   slate_loss[b] = -sum_i G_i / log2(1 + pos_i)            (caller averages: loss = mean_b, :53)
 *   dscores[b,i]  = grad_scale * d slate_loss[b] / d scores[b,i]   (NULL: forward only)
 * labels == pad marks padding (:22-24).  grad_scale is normally 1/B_global. */
int ltr_approxndcg_fwd_bwd(const float *scores, const float *labels, int B, int S, float alpha, float eps,
                           float pad, float grad_scale, float *slate_loss, float *dscores, void *stream);

/* ---- listnetLoss(y_true, y_predicted, apply_sigmoid)                        losses/listnet.py:5-16
 *   slate_loss[b] = -sum_i p_i log q_i   (p = softmax(y_true), q = softmax(y_pred); caller SUMS, :16)
 *   dscores[b,i]  = grad_scale * (q_i sum(p) - p_i);  apply_sigmoid != 0: the :13-15 variant. */
int ltr_listnet_fwd_bwd(const float *y_true, const float *y_pred, int B, int S, int apply_sigmoid,
                        float grad_scale, float *slate_loss, float *dscores, void *stream);

/* ---- lambdaLoss(...)                                                   losses/lambdaL.py:67-93 (+7-64)
 *   slate_loss[b]  = -sum over kept pairs of log_b(clamp(clamp(sigmoid(sigma d), eps)^w, eps))
 *   slate_count[b] = number of kept pairs (for reduction="mean": loss = sum(slate_loss)/sum(count))
 *   dscores[b,i]   = grad_scale * d slate_loss[b] / d scores[b,i]  (NULL: forward only)
 * k <= 0 means k=None (no truncation).  Ranks by counting, ties by index. */
int ltr_lambda_fwd_bwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                       float mu, float eps, float pad, int log_base, float grad_scale, float *slate_loss,
                       float *slate_count, float *dscores, void *stream);

/* ---- lambdaMask(..., return_losses=True)                                losses/lambdaL.py:7-60
 * losses[b, ri, rj] for ALL pairs in predicted-rank order (ri, rj = 0-based ranks), optional keep mask
 * (the boolean mask of :62, 1 byte per pair) and optional rank[b, i] = predicted rank of document i: ranks by
 * counting, ties by index (the lower index first); padded documents rank after every real one, among themselves
 * by index.  A pair with a padded document holds the same expression with that document's score -inf, gain 0 and
 * clamped label 0 (d = clamp(s_i - s_j, +-1e8), NaN -> 0): max(w log_b(eps), log_b(eps)) when the first document
 * is padded, 0 when only the second is, w log_b(1/2) when both are; keep is 0 there.  Every entry is written. */
int ltr_lambda_pairs_fwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                         float mu, float eps, float pad, int log_base, float *losses, uint8_t *keep,
                         int32_t *rank, void *stream);
/* Backward of the above: dscores[b,i] = sum_{pairs} grad_losses[b,ri,rj] * d losses[b,ri,rj] / d scores[b,i]. */
int ltr_lambda_pairs_bwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                         float mu, float eps, float pad, int log_base, const float *grad_losses,
                         float *dscores, void *stream);

/* ---- torch.sum(lambdaMask(..., return_losses=True), dim=1)        losses/riskLosses/riskLosses.py:72-83,192-203,302-310
 * The only thing the risk losses take from the pair matrix is its column sums c[b, rj] = sum_ri losses[b, ri, rj]
 * (rj = 0-based predicted rank): computed without materialising [B,S,S].  The backward takes d L / d c[B,S]. */
int ltr_lambda_colsum_fwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                          float mu, float eps, float pad, int log_base, float *colsum, void *stream);
int ltr_lambda_colsum_bwd(const float *scores, const float *labels, int B, int S, int scheme, int k, float sigma,
                          float mu, float eps, float pad, int log_base, const float *grad_colsum, float *dscores,
                          void *stream);
/* The same column sums for EVERY system of a Lambda-type risk loss in ONE launch (losses/riskLosses/riskLosses.py:63-83, :183-203,
 * :294-310): system 0 = the model (y_pred), 1..n_base = the baseline rankers (y_base [B][S][n_base], NULL when n_base == 0),
 * n_base + 1 = the ideal ranking (the labels as scores).  The label vector and every score vector are soft-maxed over the slate first
 * (:65-70, torch.softmax(dim=1)) inside the kernel.  colsum [n_base + 2][B][S]. */
int ltr_lambda_colsum_sys_fwd(const float *y_pred, const float *y_true, const float *y_base, int B, int S, int n_base, int scheme,
                              int k, float sigma, float mu, float eps, float pad, int log_base, float *colsum, void *stream);
/* Backward of system 0 w.r.t. the RAW y_pred (pair backward on the soft-maxed vectors, then the softmax's Jacobian):
 * grad_colsum [B][S] = d L / d colsum[0] -> dy_pred [B][S]. */
int ltr_lambda_colsum_sys_bwd(const float *y_pred, const float *y_true, int B, int S, int scheme, int k, float sigma, float mu,
                              float eps, float pad, int log_base, const float *grad_colsum, float *dy_pred, void *stream);
/* The same backward with d L / d colsum[0][b][j] = jac[b][j] * coef[b * coef_stride] formed inside the launch: jac = d mat[b][0] / d colsum
 * (ltr_risk_matrix_fwd / ltr_lambda_risk_model_fwd), coef = the model column of the tail's d L / d mat, read in place (coef_stride = the
 * matrix row length). */
int ltr_lambda_colsum_sys_bwd_coef(const float *y_pred, const float *y_true, int B, int S, int scheme, int k, float sigma, float mu,
                                   float eps, float pad, int log_base, const float *jac, const float *coef, int coef_stride, float *dy_pred,
                                   void *stream);
/* A Lambda-type risk matrix with the constant systems cached (the fused risk step's baseline columns): per query b, cache[b * cache_stride ..]
 * = [n_cached matrix entries (baselines, ideal ranking, ones column) | the ideal ranking's column sums [S]].  One launch: the MODEL's
 * column sums (softmaxes inside, as ltr_lambda_colsum_sys_fwd system 0), its effectiveness against the cached ideal column sums
 * (lt 1 / 2 / 3, as ltr_risk_matrix_fwd mode 1), jac [B][S] = d mat[b][0] / d colsum, and the row mat[b] = [model | cached entries]
 * ([B][1 + n_cached]).  Bitwise the matrix of ltr_lambda_colsum_sys_fwd + ltr_risk_matrix_fwd.  2 <= S <= 2048. */
int ltr_lambda_risk_model_fwd(const float *y_pred, const float *y_true, const float *cache, int cache_stride, int n_cached, int B, int S,
                              int scheme, int k, float sigma, float mu, float eps, float pad, int log_base, int lt, float *mat, float *jac,
                              void *stream);

/* ---- zRisk / geoRisk(mat, alpha, requires_grad, i)          losses/riskLosses/riskFunctions.py:4-22 / :25-33
 * mat[Q][n_systems]: effectiveness of every system (column) on every query (row); col = the system under test
 * (negative counts from the end, like the reference's i=-1).
 *   LTR_RISK_Z  : value[0] = sum_q d_q (1 + alpha [d_q < 0]),  d_q = (mat[q,col] - e_q)/sqrt(e_q),
 *                 e_q = (sum_q mat[q,col]) (sum_j mat[q,j]) / sum(mat)
 *   LTR_RISK_GEO: value[0] = sqrt(mean_q mat[q,col] * Phi(zRisk / Q))
 *   dmat[Q][n_systems] (NULL: forward only) = d value / d mat, analytic (the [d_q < 0] indicator carries none).
 * One workgroup, fp64 accumulation, fixed summation order. */
enum { LTR_RISK_Z = 0, LTR_RISK_GEO = 1,
       LTR_RISK_ZERO_GUARD = 4 };  /* OR-ed in: e_q == 0 contributes 0 and the (1 + alpha) weight keys on the raw residual --
                                      the numpy metric's rules, utils/metrics.py:26-36 (getGeoRiskDefault) */
int ltr_risk_fwd_bwd(const float *mat, int Q, int n_systems, int col, float alpha, int kind, float *value,
                     float *dmat, void *stream);

/* ---- tRisk tail                                            losses/riskLosses/riskLosses.py:278-291, :332-345
 *   delta_q = (model[q] - baseline[q]) (1 + alpha [model[q] < baseline[q]]);  value[0] = mean(delta)/std(delta)
 *   (unbiased std, torch.std);  dmodel / dbaseline [Q] (may be NULL) = d value / d model, d baseline. */
int ltr_trisk_fwd_bwd(const float *model, const float *baseline, int Q, float alpha, float *value, float *dmodel,
                      float *dbaseline, void *stream);

/* The tail of a geoRisk (kind 1) / zRisk (kind 0) loss in one launch (riskLosses.py:47-60, :118-125, :170-180, :237-244): optional
 * flip mat' = -mat + max(mat), risk of column 0 and (strategies 2 / 3) of the last column, strategy 1: f R0, 2: f (R1 - R0)
 * [zquirk != 0: f R1 - R0, the reference's precedence in zRiskListnetLoss :176], 3: f (R1 - R0)^2; value [1] and dmat [Q][n] =
 * d value / d mat (NULL = not wanted; the max passes its gradient to the maximal entries, evenly among ties). */
int ltr_risk_tail_fwd_bwd(const float *mat, int Q, int n_systems, float alpha, int kind, int strategy, int flip, float factor,
                          int zquirk, float *value, float *dmat, void *stream);

/* The tail of a tRisk loss in one launch (riskLosses.py:269-291, :332-345): mat [Q][2] = (model, baseline) per query; optional flip
 * mat' = -mat + max(mat) (transformation 1); value [1] = factor * mean(delta) / std(delta) as ltr_trisk_fwd_bwd; dmat [Q][2] (NULL = not
 * wanted) = d value / d mat. */
int ltr_trisk_tail_fwd_bwd(const float *mat, int Q, float alpha, int flip, float factor, float *value, float *dmat, void *stream);

/* The [queries x systems] effectiveness matrix of the six risk-sensitive losses in ONE launch (losses/riskLosses/riskLosses.py:8-49,
 * :63-117, :128-169, :183-236, :247-276, :294-330), mat [B][1 + n_rest + (ideal != 0)] row-major: column 0 the model, then the
 * baseline rankers, optionally the ideal ranking (the reference vector itself); and jac [B][S] = d mat[b][0] / d x0[b][j] (NULL = not
 * wanted) -- the only gradient the losses need.
 *   mode 0 (Listnet type): ref = y_true, x0 = y_predicted, rest = y_baselines [B][S][n_rest]; each vector is soft-maxed over the slate
 *     (:10-12), then lt 1: sum (t p - t^2)^2, 2: cosine(t, p), 3: (sum t p - sum t^2)^2.
 *   mode 1 (Lambda type): ref, x0, rest [n_rest][B][S] are lambdaMask column sums (ltr_lambda_colsum_fwd), taken as they are;
 *     lt 1: sum (x - t)^2, 2: cosine(t, x), 3: (sum x - sum t)^2.
 *   mode 2 (tRiskListnetLoss, :247-276): as mode 0 except lt 2 = cosine(t^2, t p), the cosine of the products.
 * The caller applies the `-mat + max(mat)` flip of lt 1 / 3 (:47-49; a whole-matrix maximum).  S <= 2048. */
int ltr_risk_matrix_fwd(const float *ref, const float *x0, const float *rest, int B, int S, int n_rest, int mode, int lt, int ideal,
                        float *mat, float *jac, void *stream);
/* As ltr_risk_matrix_fwd; ones != 0 appends one more column of 1.0 (geoRiskLambdaLoss's ideal ranking under transformation 2,
 * riskLosses.py:106): mat [B][1 + n_rest + (ideal != 0) + (ones != 0)]. */
int ltr_risk_matrix_rows_fwd(const float *ref, const float *x0, const float *rest, int B, int S, int n_rest, int mode, int lt, int ideal,
                             int ones, float *mat, float *jac, void *stream);
/* As ltr_risk_matrix_fwd with the constant columns given: mat[b] = [model | cached[b * cache_stride + 0 .. n_cached)], only the model's
 * entry (and jac) computed.  mode 0 / 2 (Listnet type); the cached entries come from an earlier ltr_risk_matrix_fwd call. */
int ltr_risk_matrix_cached_fwd(const float *ref, const float *x0, const float *cached, int cache_stride, int B, int S, int n_cached,
                               int mode, int lt, float *mat, float *jac, void *stream);
/* dscores[b][j] = jac[b][j] * dmat[b * dmat_stride]: the scores gradient of a risk loss from the model column of d L / d mat. */
int ltr_risk_scores_grad(const float *jac, const float *dmat, int dmat_stride, int B, int S, float *dscores, void *stream);
/* The two tails over an all-gathered, per-rank padded matrix (data-parallel risk step): n_blocks blocks of (1 + block_rows * n) floats,
 * block k = its valid row count (as a float), then block_rows rows.  The valid rows, in block order, are the matrix; padded rows are
 * neither read nor written, and the sums run in the order of the dense matrix (same bits as ltr_risk_tail_fwd_bwd /
 * ltr_trisk_tail_fwd_bwd on it).  dmat has the blocks' layout.  n_blocks <= 1024. */
int ltr_risk_tail_blocks_fwd_bwd(const float *blocks, int n_blocks, int block_rows, int n_systems, float alpha, int kind, int strategy,
                                 int flip, float factor, int zquirk, float *value, float *dmat, void *stream);
int ltr_trisk_tail_blocks_fwd_bwd(const float *blocks, int n_blocks, int block_rows, float alpha, int flip, float factor, float *value,
                                  float *dmat, void *stream);

/* ---- mNdcg / ndcg / dcg / torchNdcg                                            utils/metrics.py:48-104
 * Per-query NDCG@k on the device (the reference loops over queries in Python after every epoch,
 * main_batch_execution.py:173-200).  y_true, y_score: [Q][S] fp32.  k is clamped to S (:54-55).
 *   gains: LTR_GAINS_LINEAR (y) | LTR_GAINS_EXPONENTIAL (2^y - 1)                                   (:57-62)
 *   no_relevant != 0: a query whose ideal DCG is 0 scores 1.0, else 0.0                              (:70-71)
 *   reverse_ties == 0: tied scores rank lower index first (Python's stable sorted(reverse=True), :51 -- the default
 *   path); != 0: higher index first (np.argsort(...)[::-1] under a stable argsort, :53).
 * ndcg[Q] and dcg[Q] (either may be NULL) are fp64, like the reference's numpy results; dcg = the un-normalised
 * DCG@k of :48-65.  torchNdcg(k) (:83-104) = exponential, no_relevant = 0. */
enum { LTR_GAINS_LINEAR = 0, LTR_GAINS_EXPONENTIAL = 1 };
int ltr_ndcg_at_k(const float *y_true, const float *y_score, int Q, int S, int k, int gains, int no_relevant,
                  int reverse_ties, double *ndcg, double *dcg, void *stream);

/* =====================================================================================================
 * Ragged batches: queries of unequal length, no padding (a LETOR file as distributed: utils/dataset.py:44-69 builds per-query
 * lists, utils/metrics.py:77-80 loops over them).  scores / labels / dscores are [n_docs]; offsets [Q + 1] (int64, device,
 * ascending, offsets[0] = 0): query q owns rows offsets[q] .. offsets[q + 1] - 1, 1 .. LTR_MAX_SLATE of them.  slate_loss,
 * slate_count, ndcg and dcg are indexed by QUERY id, dscores by document row.
 *   queries / n_queries : the query ids this launch handles (int32, device); queries == NULL: 0 .. n_queries - 1.
 *   s_max               : an upper bound of the listed queries' lengths; launch geometry and LDS size come from it as the
 *                         rectangular entry point derives them from S.
 * The loss launches take ONE length tier at a time: every listed query has next_pow2(length) == next_pow2(s_max) (that power of
 * two fixes threads per slate, row lanes / column groups and every barrier count, so slates of unequal length can share a
 * workgroup).  A caller covers a batch with one launch per occupied tier (ltr_mi355x.ragged.RaggedSlates builds the lists).  The
 * offsets live on the device and are not read by the host: a listed query outside the tier is not computed -- its slate_loss /
 * ndcg slot becomes NaN, its count 0, its dscores rows stay untouched.  ltr_ndcg_at_k_ragged takes any lengths <= s_max.
 * Queries that are not listed keep their slots and rows untouched.  With all listed lengths equal to S the results are the bits
 * of the rectangular entry point at (n_queries, S).  Each loss is the reference's loss on every query as a batch of one; the
 * caller combines slate_loss as for the rectangular twin (mean / sum / sum over total count).  k truncates on each query's own
 * ranks.  n_queries < 0, s_max outside 1 .. LTR_MAX_SLATE: LTR_ERR_SHAPE. */
int ltr_approxndcg_ragged_fwd_bwd(const float *scores, const float *labels, const int64_t *offsets, const int32_t *queries,
                                  int n_queries, int s_max, float alpha, float eps, float pad, float grad_scale, float *slate_loss,
                                  float *dscores, void *stream);
int ltr_listnet_ragged_fwd_bwd(const float *y_true, const float *y_pred, const int64_t *offsets, const int32_t *queries,
                               int n_queries, int s_max, int apply_sigmoid, float grad_scale, float *slate_loss, float *dscores,
                               void *stream);
int ltr_lambda_ragged_fwd_bwd(const float *scores, const float *labels, const int64_t *offsets, const int32_t *queries,
                              int n_queries, int s_max, int scheme, int k, float sigma, float mu, float eps, float pad,
                              int log_base, float grad_scale, float *slate_loss, float *slate_count, float *dscores,
                              void *stream);
int ltr_ndcg_at_k_ragged(const float *y_true, const float *y_score, const int64_t *offsets, const int32_t *queries, int n_queries,
                         int s_max, int k, int gains, int no_relevant, int reverse_ties, double *ndcg, double *dcg, void *stream);

/* ---- The six risk-sensitive losses on a ragged batch               losses/riskLosses/riskLosses.py:8-49, :63-117, :128-169, :183-236,
 * :247-276, :294-330 behind main_batch_execution.py:140-165.  Entry mat[q][sys] of the effectiveness matrix is computed from query
 * q's documents alone (softmaxes over its own slate, then a sum over the slate or over its predicted ranks), so row q is the row the
 * reference computes for q inside any batch of queries of q's length, before the flip; the rows of all queries form one dense
 * [Q][n_systems] matrix for the unchanged tails (ltr_risk_tail_fwd_bwd, ltr_trisk_tail_fwd_bwd and their *_blocks_* forms).
 * offsets / queries / n_queries / s_max as above; n_docs = offsets[Q], the documents of the whole batch (host value: rows past it are
 * never touched).  With all lengths equal to S every entry below gives the bits of its rectangular twin at (n_queries, S).
 *
 * ltr_risk_matrix_ragged_fwd: ltr_risk_matrix_rows_fwd (cached == NULL) / ltr_risk_matrix_cached_fwd (cached != NULL: n_rest cached
 * entries per row at cached[q * cache_stride], ideal = ones = 0) with ref / x0 [n_docs], rest [n_docs][n_rest] (modes 0, 2;
 * riskLosses.py:10-46, :249-268) or ref / x0 / rest ragged column sums, system k at rest[(k - 1) * n_docs] (mode 1; :71-106, :205-226,
 * :312-322).  ONE launch for any lengths 1 .. s_max (256 threads per query whatever its length: no tier).  mat [Q][ld] is indexed by
 * query id, jac [n_docs] by document row.  A listed query outside 1 .. s_max gets a NaN model entry, nothing else of it is touched. */
int ltr_risk_matrix_ragged_fwd(const float *ref, const float *x0, const float *rest, const int64_t *offsets, const int32_t *queries,
                               int n_queries, int s_max, int64_t n_docs, int n_rest, int mode, int lt, int ideal, int ones,
                               const float *cached, int cache_stride, float *mat, float *jac, void *stream);
/* dscores[d] = jac[d] * dmat[q(d) * dmat_stride] over the listed queries' rows (ltr_risk_scores_grad; the backward of
 * riskLosses.py:8-49 / :128-169 / :247-276 through the scores).  One launch, one workgroup per query. */
int ltr_risk_scores_grad_ragged(const float *jac, const float *dmat, int dmat_stride, const int64_t *offsets, const int32_t *queries,
                                int n_queries, int64_t n_docs, float *dscores, void *stream);
/* The Lambda forms' pair work, ONE length tier per launch like the ragged loss launches (a listed query outside the tier is not
 * computed: its rows stay untouched, ltr_lambda_risk_model_ragged_fwd poisons its model entry with NaN).
 * ltr_lambda_colsum_sys_ragged_fwd: ltr_lambda_colsum_sys_fwd (riskLosses.py:63-83, :183-203, :294-310), y_base [n_docs][n_base],
 *   colsum [n_base + 2][n_docs]; one workgroup per (system, query).
 * ltr_lambda_risk_model_ragged_fwd: ltr_lambda_risk_model_fwd (:84-106, :205-226, :312-322 for the model alone) with the cache split
 *   into cache [Q][cache_stride] (n_cached matrix entries per query) and ideal_colsum [n_docs] (the ideal ranking's column sums, by
 *   document row); mat [Q][1 + n_cached], jac [n_docs].  s_max >= 2.
 * ltr_lambda_colsum_sys_ragged_bwd_coef: ltr_lambda_colsum_sys_bwd_coef (the backward of :72-83 / :192-203 / :302-310 for system 0),
 *   d L / d colsum[0][d] = jac[d] * coef[q(d) * coef_stride] formed inside the launch. */
int ltr_lambda_colsum_sys_ragged_fwd(const float *y_pred, const float *y_true, const float *y_base, const int64_t *offsets,
                                     const int32_t *queries, int n_queries, int s_max, int64_t n_docs, int n_base, int scheme, int k,
                                     float sigma, float mu, float eps, float pad, int log_base, float *colsum, void *stream);
int ltr_lambda_risk_model_ragged_fwd(const float *y_pred, const float *y_true, const float *cache, int cache_stride,
                                     const float *ideal_colsum, int n_cached, const int64_t *offsets, const int32_t *queries,
                                     int n_queries, int s_max, int64_t n_docs, int scheme, int k, float sigma, float mu, float eps,
                                     float pad, int log_base, int lt, float *mat, float *jac, void *stream);
int ltr_lambda_colsum_sys_ragged_bwd_coef(const float *y_pred, const float *y_true, const int64_t *offsets, const int32_t *queries,
                                          int n_queries, int s_max, int64_t n_docs, int scheme, int k, float sigma, float mu, float eps,
                                          float pad, int log_base, const float *jac, const float *coef, int coef_stride, float *dy_pred,
                                          void *stream);

/* ---- ordinalLoss(y_pred[B,S,n], y_true[B,S], n, padded_value_indicator)  losses/ordinal.py:27-53
 * n_docs = B*S documents, n ordinal probabilities each.  Targets 1[y >= k] are built with the default
 * indicator -1 (ordinal.py:39), then entries whose target == pad are masked (:41-45).
 *   sums[0] = sum of masked BCE terms, sums[1] = number of documents with >= 1 unmasked target
 *   dpred[doc,k] = (p - t) / max((1-p) p, 1e-12), 0 where masked  (caller scales by 1/sums[1])
 * block_partials: workspace of 2*ltr_ordinal_num_blocks(n_docs) floats. */
int64_t ltr_ordinal_num_blocks(int64_t n_docs);
int ltr_ordinal_fwd_bwd(const float *y_pred, const float *y_true, int64_t n_docs, int n, float pad,
                        float *block_partials, float *sums, float *dpred, void *stream);

/* =====================================================================================================
 * FC scorers and the fused slate pipeline (scorer forward -> listwise loss -> scorer backward -> dW).
 *
 *   LTR_NET_DOUBLE  architeture/doubleLayer.py:54-73  fc3(drop(relu(fc2(drop(relu(fc1 x))))))  136-136-136-1
 *   LTR_NET_TRIPLE  architeture/tripleLayer.py:5-17   l3(sigmoid(l2(l1 x)))                     136-64-32-1
 *
 * Parameters are handed over exactly as the nn.Module holds them (nn.Linear: weight [out][in], bias [out]);
 * ltr_mlp_pack turns them into lane-ordered MFMA fragments once per optimizer step.  X is [n_docs][F]
 * fp32, 16-byte aligned, documents of a slate contiguous ([B][S][F] viewed as [B*S][F]).
 * Gradients come back as ONE flat fp32 buffer in nn.Module.parameters() order
 *   [W1 (H1*F) | b1 (H1) | W2 (H2*H1) | b2 (H2) | w3 (H2) | b3 (1)]
 * -- the buffer the data-parallel all-reduce runs on.  No gradient w.r.t. X is produced (the reference
 * computes one only because its drivers set requires_grad on the data, main_batch_execution.py:79).
 */
enum { LTR_NET_DOUBLE = 0, LTR_NET_TRIPLE = 1,         /* 136 input features (MSLR-WEB10K/30K) */
       LTR_NET_DOUBLE_64 = 2, LTR_NET_TRIPLE_64 = 3,    /* the same classes on 64 features (TD2003): 64-64-64-1, 64-64-32-1 */
       LTR_NET_TWO_LAYER_64H = 4,    /* 136 -> 64 -> 1, ReLU: the commented-out two-Linear DoubleLayerNet variant of
                                        architeture/doubleLayer.py:38-51 (BASELINE.json configs[0]); benchmark use.  No fc2:
                                        W2 / b2 are NULL in ltr_mlp_pack and the flat gradient is [W1 | b1 | w3 | b3].
                                        */
       LTR_NET_TRIPLE_FOLDED = 5,  /* TripleLayerNet with l2 . l1 folded into one 136 -> 32 sigmoid layer (tripleLayer.py:14-16 has
                                        no activation between them): a two-layer net [64 x 136 | 64 | 64 | 1] whose rows 32..63
                                        repeat rows 0..31 (each copy runs on half of a tile's documents).  Parameters from
                                        ltr_triple_fold, gradients back through ltr_triple_unfold_grads.  ltr_fused_step* only. */
       LTR_NET_TRIPLE_FOLDED_32 = 6,   /* the same folded network as a plain two-layer net [32 x 136 | 32 | 32 | 1] (copies = 1) for
                                        ltr_mlp_forward / _backward / _forward_save / _backward_saved. */
       LTR_NET_TRIPLE_FOLDED_32_64 = 7 }; /* TripleLayerNet on 64 features (TD2003) folded: [32 x 64 | 32 | 32 | 1], every entry
                                        point (its fused step runs on the generic pipeline). */
enum { LTR_LOSS_APPROXNDCG = 0, LTR_LOSS_LISTNET = 1 };

/* TripleLayerNet (F input features) -> its folded two-layer form, fp64 accumulation; R = 32 copies rows (copies = 2: LTR_NET_TRIPLE_FOLDED,
 * copies = 1: LTR_NET_TRIPLE_FOLDED_32 / _32_64):
 *   W1e [R][F]: rows c 32 + u = (W2 W1)[u];  b1e [R] = (W2 b1 + b2)[u];  w3e [R] = w3[u]  (u < 32, c < copies).
 * Once per step (weights change every step): 32 x 64 x (F + 1) multiply-adds. */
int ltr_triple_fold(const float *W1, const float *b1, const float *W2, const float *b2, const float *w3, int F, int copies, float *W1e,
                    float *b1e, float *w3e, void *stream);
/* The flat gradient of the folded net, g2 = [dW1e R x F | db1e R | dw3e R | db3], -> TripleLayerNet's flat gradient
 * [dW1 64 x F | db1 64 | dW2 32 x 64 | db2 32 | dw3 32 | db3]: with G[u] = sum_c dW1e[c 32 + u], gb[u] = sum_c db1e[c 32 + u],
 *   dW1 = W2^T G, db1 = W2^T gb, dW2 = G W1^T + gb b1^T, db2 = gb, dw3[u] = sum_c dw3e[c 32 + u].  fp64 accumulation. */
int ltr_triple_unfold_grads(const float *g2, int F, int copies, const float *W1, const float *b1, const float *W2, float *flat,
                            void *stream);

/* info[0..7] = F, H1, H2, n_params, packed_floats, partial_floats (per workgroup), docs_per_tile, lds_bytes */
int ltr_net_info(int net, int32_t *info);
/* Number of persistent workgroups the fused step of `net` wants on a device with n_cus compute units (one per CU; two for
 * kernels that run two 256-thread workgroups per CU).  `partials` must hold that many * partial_floats floats. */
int ltr_fused_grid(int net, int n_cus);

int ltr_mlp_pack(int net, const float *W1, const float *b1, const float *W2, const float *b2, const float *w3,
                 const float *b3, float *packed, void *stream);
/* Narrower networks on a compiled geometry (the reference's constructors take any input size: DoubleLayerNet(input_size) is
 * input_size -> input_size -> input_size -> 1, doubleLayer.py:55-60; TripleLayerNet(N_features) is N_features -> 64 -> 32 -> 1,
 * tripleLayer.py:6-10): f / h1 / h2 are the LOGICAL widths of the parameter tensors handed in (W1 [h1][f], W2 [h2][h1], w3 [h2]),
 * each <= the compiled width; the padded inputs / hidden units get zero weights.  The caller pads X rows with zeros to the
 * compiled feature count.  ltr_mlp_reduce_grads_sub writes the flat gradient in the LOGICAL layout
 * [W1 (h1*f) | b1 (h1) | W2 (h2*h1) | b2 (h2) | w3 (h2) | b3 (1)]. */
int ltr_mlp_pack_sub(int net, int f, int h1, int h2, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *w3, const float *b3, float *packed, void *stream);
int ltr_mlp_reduce_grads_sub(int net, int f, int h1, int h2, const float *partials, int grid, float *flat_grad, void *stream);

/* Scorer forward: scores[n_docs] = net(X).  dropout != 0 applies training-mode Dropout(0.5) after each ReLU
 * (doubleLayer.py:60-65) from the counter-based stream (seed, document, feature); keep1/keep2, when non-NULL,
 * are explicit keep masks [n_docs][H1] / [n_docs][H2] (bytes, != 0 keeps) used INSTEAD of the generator
 * (parity tests).  grid = number of persistent workgroups (normally the CU count). */
int ltr_mlp_forward(int net, const float *X, int64_t n_docs, const float *packed, int dropout, uint64_t seed,
                    const uint8_t *keep1, const uint8_t *keep2, float *scores, int grid, void *stream);

/* out[doc][n] (bytes, n < H) = keep bit of dropout layer `layer` (0 after fc1, 1 after fc2) that the pipeline
 * kernels derive from (seed, document index, feature index): the counter-based replacement for the torch
 * CPU generator stream behind nn.Dropout (doubleLayer.py:60), which cannot be reproduced on the device. */
int ltr_dropout_keep_mask(uint64_t seed, int layer, int64_t n_docs, int H, uint8_t *out, void *stream);
/* Dropout probabilities other than the reference's 0.5 (a caller that sets `net.dropout.p`): every `dropout` argument below is
 * 0 (off), 1 (on, p = 0.5) or `1 | (bits of the float p with its lowest bit cleared)` (on, that p; kept units scaled by
 * 1 / (1 - p)).  p = 0.5 draws one hash bit per hidden unit, any other p 16 bits (unit dropped when they are < round(p * 65536)).
 * Only the forward kernels carry the 16-bit stream: with such a p use ltr_mlp_forward / ltr_mlp_forward_save and
 * ltr_mlp_backward_saved (the saved activations make the backward independent of the stream); ltr_mlp_backward and the fused
 * steps return LTR_ERR_PARAM for it unless explicit keep masks are passed.  ltr_dropout_keep_mask_p exports the stream. */
int ltr_dropout_keep_mask_p(uint64_t seed, int layer, int64_t n_docs, int H, float p, uint8_t *out, void *stream);

/* Scorer backward given dL/dscores[n_docs]: recomputes the forward from X (same seed/masks) and leaves one
 * gradient partial per workgroup in `partials` (grid * partial_floats floats); ltr_mlp_reduce_grads then sums
 * them in a fixed order into the flat parameter gradient. */
int ltr_mlp_backward(int net, const float *X, int64_t n_docs, const float *packed, int dropout, uint64_t seed,
                     const uint8_t *keep1, const uint8_t *keep2, const float *dscores, float *partials, int grid,
                     void *stream);
int ltr_mlp_reduce_grads(int net, const float *partials, int grid, float *flat_grad, void *stream);

/* The same forward / backward pair with ONE forward (what autograd does in the reference, main_batch_execution.py:128-170):
 * ltr_mlp_forward_save also writes the post-activation hidden layers h1 / h2 (dropout applied) of every document to `acts`
 * (ltr_mlp_acts_floats(net, n_docs) floats, 16-byte aligned: one lane-ordered 1 KiB fragment per 16-document tile and 16
 * features), ltr_mlp_backward_saved reads them back instead of recomputing fc1 / fc2 (the backward kernel is bound by the
 * fp32 matrix pipe, the round trip costs HBM bandwidth it does not use).  Used for slate lengths the one-launch fused
 * step does not cover (BASELINE config 3: slate 512).  `dropout` only selects the ReLU-dropout slope (2) of the backward.
 */
int64_t ltr_mlp_acts_floats(int net, int64_t n_docs);      /* < 0: LTR_ERR_* */
int ltr_mlp_forward_save(int net, const float *X, int64_t n_docs, const float *packed, int dropout, uint64_t seed,
                         const uint8_t *keep1, const uint8_t *keep2, float *scores, float *acts, int grid, void *stream);
int ltr_mlp_backward_saved(int net, const float *X, int64_t n_docs, const float *packed, int dropout, const float *acts,
                           const float *dscores, float *partials, int grid, void *stream);

/* One fused training pass over B slates of S documents (S in {32, 64, 128}): scorer forward, per-slate loss
 * (LTR_LOSS_*; labels [B][S]), loss backward, scorer backward -- scores never leave the CU, X is read once.
 *   slate_loss[b]  : per-slate loss (caller reduces: mean for approxNDCG, sum for ListNet)
 *   partials       : per-workgroup partials of d (sum_b grad_scale * slate_loss[b]) / d params, to be summed by
 *                    ltr_mlp_reduce_grads (grad_scale = 1/B_global for a mean)
 * main_batch_execution.py:128-170 is the reference call chain this replaces. */
int ltr_fused_step(int net, int loss_kind, const float *X, const float *labels, int B, int S, const float *packed,
                   int dropout, uint64_t seed, const uint8_t *keep1, const uint8_t *keep2, float alpha, float eps,
                   float pad, int apply_sigmoid, float grad_scale, float *slate_loss, float *partials, int grid,
                   void *stream);

/* Diagnostics: in a build compiled with -DLTR_STAMPS the pipeline kernels write s_memtime stamps at their phase
 * boundaries for workgroup-local tile `tile` to buf[grid][8][16] (uint64); returns 1 in such a build, 0 otherwise
 * (the stamps are then compiled out).  buf = NULL disables. */
int ltr_debug_set_stamps(void *buf, int tile);

/* The same fused pass with lambdaLoss (losses/lambdaL.py:67-93; the loss main_batch_execution.py:135 trains
 * with: weighing_scheme="ndcgLoss2PP_scheme").  scheme/k/sigma/mu/eps/log_base as in ltr_lambda_fwd_bwd;
 * slate_loss[b] = -sum of the kept pair terms, slate_count[b] (may be NULL) = kept pairs.  reduction="sum":
 * grad_scale = 1; a "mean" is obtained by dividing loss and flat gradient by the (global) pair count. */
int ltr_fused_step_lambda(int net, const float *X, const float *labels, int B, int S, const float *packed, int dropout,
                          uint64_t seed, const uint8_t *keep1, const uint8_t *keep2, int scheme, int k, float sigma,
                          float mu, float eps, float pad, int log_base, float grad_scale, float *slate_loss,
                          float *slate_count, float *partials, int grid, void *stream);

/* =====================================================================================================
 * FC-only make_model rankers (csrc/ltr_linear.hip): LTRModel = FCModel -> OutputLayer with no transformer, d_output = 1 and no
 * active dropout.  FCModel (architeture/multiLayer.py:13-51) and OutputLayer (:94-124) hard-wire nn.Identity activations, so the
 * network make_model builds (:127-149) is ONE affine map of h_0 (x, or LayerNorm(x) with input_norm):
 *   v_L = w_o, v_{i-1} = v_i W_i, w_eff = v_0, b_eff = b_o + sum_i v_i . b_i.
 * One training step: ltr_linear_fold -> (ltr_linear_fused_step | ltr_linear_scores + loss kernel + ltr_linear_grad_partials)
 * -> ltr_linear_unfold_grads.  Exact fp32 on the documents, fp64 in the fold / unfold chains; no atomics.
 *
 * `params` (HOST array of device pointers) in LTRModel._ltr_params() order: [gamma, beta] if input_norm, then W_1 [n_1][F], b_1, ...,
 * W_L [n_L][n_{L-1}], b_L, then w_o [1][n_L], b_o [1].  sizes[i] = n_{i+1} (host, n_layers entries; n_layers = 0: OutputLayer
 * only).  ws: ltr_linear_ws_doubles() fp64, device, shared by the fold and the unfold of one step. */
#define LTR_LINEAR_MAX_LAYERS 16
int64_t ltr_linear_ws_doubles(int n_layers, int F, const int *sizes);     /* < 0: shape rejected */
/* weff[F + 2] = [w_eff (o gamma with input_norm) | b_eff (+ w_eff . beta) | sum of the first F]   multiLayer.py:13-51, :94-124 */
int ltr_linear_fold(int n_layers, int F, const int *sizes, int input_norm, const float *const *params, double *ws, float *weff,
                    void *stream);
/* partials [grid][F + 1] = per-workgroup [sum_d ds_d xhat_d | sum_d ds_d] (fixed-order sum here) -> the flat gradient in _ltr_params()
 * order: H_0 = Ghat (gamma o Ghat + beta G_1), H_i = W_i H_{i-1} + b_i G_1, dW_i = v_i H_{i-1}^T, db_i = v_i G_1, dw_o = H_L,
 * db_o = G_1, dgamma = w_eff o Ghat, dbeta = w_eff G_1.  ws as left by ltr_linear_fold on the same parameters.   multiLayer.py:127-149 */
int ltr_linear_unfold_grads(int n_layers, int F, const int *sizes, int input_norm, const float *const *params, const float *partials,
                            int grid, double *ws, float *flat, void *stream);
/* scores[n] = weff . x + weff[F] (input_norm: rstd (weff . (x - mean)) + weff[F]; stats[n][2] = (mean, rstd)).  F <= 1024.
 * multiLayer.py:36-46 + :107-113 on the folded vector. */
int ltr_linear_scores(const float *X, int64_t n, int F, const float *weff, int input_norm, float *scores, float *stats, void *stream);
/* partials[g] = [sum_d ds_d xhat_d | sum_d ds_d] over workgroup g's contiguous document range (grid workgroups).  F <= 1024. */
int ltr_linear_grad_partials(const float *X, int64_t n, int F, const float *dscores, const float *stats, int input_norm, float *partials,
                             int grid, void *stream);
/* 1 when the one-launch step takes (F, S): S in {32, 64, 128}, F % 4 == 0, F <= 256. */
int ltr_linear_fused_supported(int F, int S);
/* One launch: scores, per-slate loss (loss_kind LTR_LOSS_APPROXNDCG / LTR_LOSS_LISTNET / 2 = lambdaLoss with scheme, k, sigma, mu,
 * lambda_eps, log_base as in ltr_lambda_fwd_bwd), d loss / d s and the gradient partials [grid][F + 1] of
 * sum_b grad_scale slate_loss[b].  slate_count (lambdaLoss, may be NULL): kept pairs per slate.  X and weff 16-byte aligned.
 * main_batch_execution.py:128-170 with net_structure = allrank is the call chain this replaces. */
int ltr_linear_fused_step(int loss_kind, const float *X, const float *labels, int B, int S, int F, const float *weff, int input_norm,
                          float alpha, float eps, float pad, int apply_sigmoid, int scheme, int k, float sigma, float mu,
                          float lambda_eps, int log_base, float grad_scale, float *slate_loss, float *slate_count, float *partials,
                          int grid, void *stream);
/* The six risk-sensitive losses on the folded network (riskLosses.py:8-49, :128-169, :247-276 behind main_batch_execution.py:93-94,
 * :140-164 with net_structure = allrank).  Entry mat[q][0] of the effectiveness matrix depends on slate q's scores alone, so with
 * j_d = d mat[q][0] / d s_d the slate's whole contribution to [Ghat | G_1] is c_q R_q, R_q = [sum_d j_d xhat_d | sum_d j_d], where
 * c_q = d value / d mat[q][0] comes out of the tail (ltr_risk_tail_fwd_bwd / ltr_trisk_tail_fwd_bwd or their *_blocks_* forms).
 *
 * ltr_linear_risk_rows: the Listnet forms in one pass over X where ltr_linear_fused_supported(F, S) holds.  Scores from weff, then per
 * slate the model's entry as ltr_risk_matrix_cached_fwd computes it (mode 0: geoRisk / zRisk Listnet, mode 2: tRiskListnetLoss; lt 1 / 2 / 3;
 * fp32 elementwise, fp64 sums) into mat[q * n_systems], cached[q * cache_stride + 0 .. n_cached) copied to mat[q * n_systems + 1 ..],
 * and R [B][F + 1].  X and weff 16-byte aligned.  B < 1, or (F, S) outside the supported set: LTR_ERR_SHAPE, nothing launched. */
int ltr_linear_risk_rows(const float *X, const float *labels, int B, int S, int F, const float *weff, int input_norm, int mode, int lt,
                         const float *cached, int cache_stride, int n_cached, float *mat, int n_systems, float *R, int grid,
                         void *stream);
/* partials [grid][F + 1] = per-workgroup sum_q dmat[q * dmat_stride] R[q] over a contiguous range of slates, in order: what
 * ltr_linear_unfold_grads reduces.  dmat is read in place at the matrix's row stride, as ltr_risk_scores_grad reads it (the backward of
 * riskLosses.py:8-49 / :128-169 / :247-276 through the scores, main_batch_execution.py:167-168).  F <= 1024; B < 1: LTR_ERR_SHAPE. */
int ltr_linear_risk_combine(const float *R, const float *dmat, int dmat_stride, int B, int F, float *partials, int grid, void *stream);
/* Workgroups of ltr_linear_fused_step / ltr_linear_grad_partials on a device with n_cus compute units (2 per CU). */
int ltr_linear_grid(int n_cus);

/* =====================================================================================================
 * FC scorers with 137 .. 1024 input features (csrc/ltr_wide.hip): the public LETOR collections beyond the reference's two
 * (Istella 220, Yahoo LTRC 700).  The slate pipeline above holds a 128-document tile of at most 136 features in LDS; these widths
 * run as a chain of launches on one exact-fp32 GEMM.  No LTR_F16X2 form: both libraries compile the same code.
 *
 * ---- ltr_gemm_f32: the exact-fp32 sibling of ltr_enc_gemm_bf16 (ltr_encoder.h), on v_mfma_f32_16x16x4_f32 -- every output is
 * a k-ordered fp32 fmaf chain.       C[m][n] = sum_k A(m,k) * B(n,k)        m < M, n < N, k < K
 *   A(m,k) = a_kmajor ? A[k*lda + m] : A[m*lda + k]   (same for B); no operand is ever transposed in memory:
 *        forward   z = x W^T      A = x [T][K],  B = W [N][K]                   (0, 0)      doubleLayer.py:62-66, tripleLayer.py:14-16
 *        d h       = dz W         A = dz [T][N], B = W [N][K] k-major           (0, 1)
 *        d W       = dz^T x       A = dz [T][N] k-major, B = x [T][K] k-major   (1, 1), split over T
 *   64 x 64 output tile per 256-thread workgroup, 16-wide k tiles staged through LDS.  M >= 0 and K >= 1 of any size (64-bit
 *   indices), 1 <= N <= 1024, odd extents included.  An operand is read 16 bytes per lane when its base is 16-byte aligned and its
 *   leading dimension a multiple of 4, else 4 bytes per lane; rows and k outside the extents are zero-filled in LDS, never read.
 *   Epilogue, in this order (all optional): + bias[n]; act (LTR_GEMM_ACT_*; the sigmoid is the correctly rounded 1 / (1 + exp(-v)));
 *   gate through the saved post-activation tensor g = gate[m*ldg + n] -- LTR_GEMM_GATE_RELU: v = g > 0 ? v * gate_scale : 0 (the
 *   ReLU + dropout backward), LTR_GEMM_GATE_SIGMOID: v * (g * (1 - g)); dropout with the SCORERS' keep stream: `dropout` is the
 *   drop code of the entries above (0, 1 or 1 | bits of p), unit (doc = m, n) of layer `drop_layer` is kept exactly where
 *   ltr_dropout_keep_mask / ltr_dropout_keep_mask_p (seed, drop_layer) say so, or where keep[m*N + n] != 0 when `keep` is given
 *   (bytes; used INSTEAD of the stream); kept values are multiplied by the fp32 value 1 / (1 - p); store fp32 (ldc).
 *   splits > 1: a split over K in slices of ceil(ceil(K / 16) / splits) * 16; slice z writes its raw partial to C + z*M*ldc (no
 *   epilogue), a slice past the end of K writes zeros -- reduce with ltr_enc_sum_partials.  No atomics: same inputs, same bits.
 *   NULL A / B / C (or a gate kind without gate): LTR_ERR_NULL; extents or leading dimensions out of range, splits outside
 *   1 .. 1024: LTR_ERR_SHAPE; unknown act / gate kind, drop_layer outside 0 .. 1, p outside (0, 1): LTR_ERR_PARAM; a pointer not
 *   4-byte aligned: LTR_ERR_ALIGN; M == 0: LTR_OK without a launch. */
enum { LTR_GEMM_ACT_NONE = 0, LTR_GEMM_ACT_RELU = 1, LTR_GEMM_ACT_SIGMOID = 2 };
enum { LTR_GEMM_GATE_NONE = 0, LTR_GEMM_GATE_RELU = 1, LTR_GEMM_GATE_SIGMOID = 2 };
typedef struct ltr_gemm_f32_desc {
    const float *A, *B;
    int64_t M, N, K, lda, ldb, ldc;
    int32_t a_kmajor, b_kmajor, splits, act;
    float *C;
    const float *bias;
    const float *gate;
    int64_t ldg;
    int32_t gate_kind;
    float gate_scale;
    int32_t dropout, drop_layer;
    uint64_t seed;
    const uint8_t *keep;
} ltr_gemm_f32_desc;
int ltr_gemm_f32(const ltr_gemm_f32_desc *desc /* host pointer */, void *stream);

/* Column sums of an fp32 [T][N] tensor (leading dimension ld), the bias gradients: partials[blk][n] = sum over workgroup blk's
 * contiguous row range (ceil(T / nblk) rows each, fixed order) of row_weights[t] * y[t*ld + n]; row_weights == NULL: 1 (non-NULL:
 * d w3 = sum_d ds_d h_d).  Reduce with ltr_enc_sum_partials(partials, nblk, N, ...).  1 <= N <= 1024, ld >= N, 1 <= nblk <= 65535. */
int ltr_colsum_f32(const float *y, int64_t T, int N, int64_t ld, const float *row_weights, float *partials, int nblk, void *stream);

/* ---- The training chain as two launchers, the wide counterparts of ltr_mlp_forward_save / ltr_mlp_backward_saved.  They enqueue
 * several kernels on `stream`, allocate nothing and never synchronise (capturable).
 *   LTR_WIDE_RELU3     F -> H1 -> H2 -> 1, ReLU + dropout after fc1 and fc2: DoubleLayerNet (doubleLayer.py:54-73; H1 = H2 = F there)
 *   LTR_WIDE_SIGMOID2  F -> H1 -> 1, sigmoid: TripleLayerNet (tripleLayer.py:5-17) folded by ltr_triple_fold with copies = 1
 *                      (H1 = 32); H2 is ignored
 * `params`: HOST array of device pointers W1 [H1][F], b1, [W2 [H2][H1], b2,] w3, b3 as the module holds them.  keep1 / keep2:
 * optional explicit keep masks [n_docs][H1] / [n_docs][H2], else the stream of (seed, layer 0 / 1).
 * acts (ltr_wide_acts_floats): the saved post-activation layers, row-major, dropout applied: h1 [n_docs][H1] at 0 and, for RELU3,
 *   h2 [n_docs][H2] at r4(n_docs H1), r4(x) = x rounded up to a multiple of 4;  floats = r4(n_docs H1) [+ r4(n_docs H2)].
 * ws (ltr_wide_ws_floats): RELU3: dz2 [n_docs][H2] | dz1 [n_docs][H1] | partials; SIGMOID2: dz1 | partials.
 *   floats = [r4(n_docs H2) +] r4(n_docs H1) + r4(max(grid max(H1, H2), splits(H1, F) H1 F [, splits(H2, H1) H2 H1])),
 *   splits(M, N) = clamp(ceil(grid / (ceil(M / 64) ceil(N / 64))), 1, min(ceil(max(n_docs, 1) / 64), 1024)): the slices of that
 *   weight-gradient GEMM; `grid` (1 .. 65535) is the number of workgroups a launch should fill.
 * Forward: h1 = drop(relu(X W1^T + b1)), h2 = drop(relu(h1 W2^T + b2)), scores = h2 . w3 + b3 (one wave per document).
 * Backward (reads the saved layers, never the dropout stream; `dropout` only selects the slope 1 / (1 - p); no dL/dX):
 *   dw3 = sum_d ds_d h2_d, db3 = sum_d ds_d; dz2 = (ds (x) w3) gated by h2; dW2 = dz2^T h1 (split over documents), db2 = colsum dz2;
 *   dz1 = (dz2 W2) gated by h1; dW1 = dz1^T X, db1 = colsum dz1.  flat_grad: RELU3 [W1 | b1 | W2 | b2 | w3 | b3] in parameters()
 *   order; SIGMOID2 [dW1e H1 x F | db1e H1 | dw3e H1 | db3], the g2 layout ltr_triple_unfold_grads takes.
 * Checked in this order before any launch: NULL required pointer (X, params and its entries, scores / dscores, acts, ws,
 * flat_grad): LTR_ERR_NULL; F, H1 (RELU3: H2) outside 1 .. 1024, n_docs < 0, grid outside 1 .. 65535: LTR_ERR_SHAPE; unknown kind,
 * a drop code with p outside (0, 1): LTR_ERR_PARAM; X, acts or ws not 16-byte aligned: LTR_ERR_ALIGN; n_docs == 0: LTR_OK
 * without a launch (the backward zeroes flat_grad with a memset on the stream). */
enum { LTR_WIDE_RELU3 = 0, LTR_WIDE_SIGMOID2 = 1 };
int64_t ltr_wide_acts_floats(int kind, int F, int H1, int H2, int64_t n_docs);            /* < 0: LTR_ERR_* */
int64_t ltr_wide_ws_floats(int kind, int F, int H1, int H2, int64_t n_docs, int grid);    /* < 0: LTR_ERR_* */
int ltr_wide_forward_save(int kind, int F, int H1, int H2, const float *X, int64_t n_docs, const float *const *params, int dropout,
                          uint64_t seed, const uint8_t *keep1, const uint8_t *keep2, float *scores, float *acts, void *stream);
int ltr_wide_backward_saved(int kind, int F, int H1, int H2, const float *X, int64_t n_docs, const float *const *params, int dropout,
                            const float *acts, const float *dscores, float *ws, int grid, float *flat_grad, void *stream);

/* =====================================================================================================
 * Data path in front of the pipeline.
 *
 * ---- get_data(info_dataset, type_file)                                        utils/dataset.py:33-69
 * LETOR / svmlight text ("<label> qid:<q> <fid>:<val> ... # comment") -> packed rows, HOST pointers, N host threads
 * over an mmap (n_threads <= 0: all cores).  Two calls: scan (documents, feature-id range: sklearn's zero_based="auto"
 * rule is `min id == 0 ? zero-based : one-based`), then load into caller-allocated arrays in FILE order:
 *   X[n_docs][n_features] fp32 (absent features 0; values parsed as float64 then cast, like dataset.py:63),
 *   y[n_docs] fp64 (svmlight labels are float64), qid[n_docs] (-1 if the line has none).
 * Grouping documents into queries (a new query starts where qid changes, dataset.py:54-60) is the caller's. */
int ltr_svmlight_scan(const char *path, int64_t *n_docs, int32_t *min_feature_id, int32_t *max_feature_id, int n_threads);
int ltr_svmlight_load(const char *path, int64_t n_docs, int n_features, int feature_id_base, float *X, double *y,
                      int64_t *qid, int n_threads);

/* ---- X_train[idx] / y_train[idx] / y_baseline_train[idx]                  main_batch_execution.py:112-117
 * dst[r][:] = src[idx[r]][:] for r < n_rows (device pointers; rows of row_floats fp32; idx int64, entries outside
 * [0, src_rows) leave the destination row untouched).  16-byte-per-lane copies when row_floats % 4 == 0 and both
 * bases are 16-byte aligned.  HBM-bound: every byte is read once and written once. */
int ltr_gather_rows_f32(const float *src, int64_t src_rows, const int64_t *idx, int64_t n_rows, int64_t row_floats,
                        float *dst, void *stream);

/* ---- data.slate_length (config.json) / fixed-length slates from a ragged collection          utils/dataset.py:44-69
 * The reference keeps per-query lists (dataset.py:44-69) and its config carries data.slate_length = 100, the allRank rule: every
 * query becomes one slate of S documents, a longer query sub-sampled (anew each epoch), a shorter one padded with label -1.  Here
 * that step runs on the device.  offsets / queries / n_queries as for the ragged loss launches above (queries == NULL: 0 ..
 * n_queries - 1); a query has len = 1 .. LTR_MAX_SLATE documents, 1 <= S <= LTR_MAX_SLATE.  One 256-thread workgroup per listed query.
 *
 * ltr_slates_select: rows [n_queries][S] (int64) and, when non-NULL, mask [n_queries][S] (bytes), every entry written.  Listed
 *   query i (id q) keeps k = min(len, S) documents: LTR_SLATES_FIRST its first k; LTR_SLATES_SAMPLE all of them when len <= S, else
 *   the S documents with the smallest 64-bit key (ties: the lower index), the key of local document j being, mod 2^64,
 *       z = seed ^ (q * 0xD1B54A32D192ED03 + j * 0x9E3779B97F4A7C15 + 0x8CB92BA72F3D8DD7)
 *       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  key = z ^ (z >> 31)
 *   (ranks by counting over the keys in LDS, as the loss kernels rank scores).  The kept documents fill slots 0 .. k - 1 in
 *   ascending document order: rows[i][slot] = offsets[q] + j, mask 0; slots k .. S - 1: rows -1, mask 1 (1 = padded, the
 *   convention of the encoder's padding masks).  A listed query whose length is outside 1 .. LTR_MAX_SLATE gets S padding slots.
 * ltr_slates_gather_f32: dst[i][:] = src[rows[i]][:] when 0 <= rows[i] < src_rows, else the whole row = fill (a negative index
 *   does NOT count from the end: the difference from ltr_gather_rows_f32).  Copies keep every bit (NaN payloads, -0.0).
 * ltr_slates_scatter_f32: dst[rows[i]][:] = src[i][:] for 0 <= rows[i] < dst_rows; every other dst row is left untouched.  No
 *   atomics: the caller's rows name no destination twice (select / build never repeat a non-negative row).
 *   Both: 16-byte-per-lane copies when row_floats % 4 == 0 and both bases are 16-byte aligned, else 4-byte ones.
 * ltr_slates_build: the per-batch path in ONE launch -- the selection, X_out [n_queries * S][F] (zero rows in padding slots),
 *   y_out [n_queries * S] (`pad` in padding slots), and mask / rows as ltr_slates_select writes them (either may be NULL).  Bitwise
 *   ltr_slates_select followed by ltr_slates_gather_f32 on X (fill 0) and on y (fill pad).  16-byte copies when F % 4 == 0 and X,
 *   X_out are 16-byte aligned, else 4-byte ones.  F <= 2^20.
 * NULL required pointer: LTR_ERR_NULL; n_queries < 0, S outside 1 .. LTR_MAX_SLATE, F or row_floats < 1, a negative count:
 * LTR_ERR_SHAPE; unknown mode: LTR_ERR_PARAM; then a count of 0 returns LTR_OK without a launch. */
enum { LTR_SLATES_FIRST = 0, LTR_SLATES_SAMPLE = 1 };
int ltr_slates_select(const int64_t *offsets, const int32_t *queries, int n_queries, int S, int mode, uint64_t seed, int64_t *rows,
                      uint8_t *mask, void *stream);
int ltr_slates_gather_f32(const float *src, int64_t src_rows, const int64_t *rows, int64_t n_slots, int64_t row_floats, float fill,
                          float *dst, void *stream);
int ltr_slates_scatter_f32(const float *src, const int64_t *rows, int64_t n_slots, int64_t row_floats, int64_t dst_rows, float *dst,
                           void *stream);
int ltr_slates_build(const float *X, const float *y, const int64_t *offsets, const int32_t *queries, int n_queries, int S, int F,
                     int mode, uint64_t seed, float pad, float *X_out, float *y_out, uint8_t *mask, int64_t *rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LTR_MI355X_H */
