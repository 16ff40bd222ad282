// ltr_data.hip -- the data path in front of the slate pipeline.
//
//   (1) LETOR / svmlight text -> packed fp32 rows.  The reference parses with sklearn and then walks every
//       document in Python (utils/dataset.py:34-69: `data[0][i].toarray().reshape(-1).astype(np.float32)` per
//       document, joblib-cached because it is slow).  Here: mmap + N host threads, two passes (count lines and
//       feature-id range; fill), straight into the packed [n_docs][F] layout the kernels stream.  HOST code.
//   (2) Per-epoch shuffle.  The reference gathers the whole training tensor every epoch
//       (`X_train = X_train[idx]`, main_batch_execution.py:112-117).  ltr_gather_rows_f32 is that gather on the
//       device: one coalesced 16-byte-per-lane row copy per destination row, HBM-bound (reads + writes every byte
//       once).  The slate pipeline itself can also take the permutation directly (see ltr_fused_step's callers),
//       in which case nothing is copied at all.
//   (3) Fixed-length slates from a ragged collection (config.json data.slate_length; the reference keeps per-query lists,
//       utils/dataset.py:44-69): per query the first S documents or a seeded sample of S, padding behind them, the padded
//       [B][S][F] batch, its labels, its mask and its row map in one launch (ltr_slates_build); the row map alone
//       (ltr_slates_select) with the gather / scatter that take dense tensors to ragged order and back.
#include "../../include/ltr_mi355x.h"
#include "ltr_device.h"
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------ device gather
// dst[r][:] = src[idx[r]][:], rows of `row_f4` float4s.  One workgroup handles kRowsPerBlock destination rows;
// lanes sweep a row in 16-byte pieces (fully coalesced on both sides).  Negative indices count from the end like torch
// indexing (idx + src_rows); an index still out of range yields a ZERO row (torch raises a device-side assert there).
// kWrap = false (ltr_slates_gather_f32): a negative index is out of range too, and such a row is `fill`.
constexpr int kGatherThreads = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool kWrap>
__global__ void __launch_bounds__(kGatherThreads)
gather_rows_kernel(const f32x4 *__restrict__ src, const int64_t *__restrict__ idx, int64_t n_rows, int64_t src_rows,
                   int row_f4, float fill, f32x4 *__restrict__ dst) {
    const int64_t total = n_rows * row_f4;
    for (int64_t e = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kGatherThreads) {
        const int64_t r = e / row_f4;
        const int c = (int)(e - r * row_f4);
        int64_t s = idx[r];
        if (kWrap && s < 0) s += src_rows;
        dst[e] = s >= 0 && s < src_rows ? __builtin_nontemporal_load(src + s * row_f4 + c) : f32x4{fill, fill, fill, fill};
    }
}

// Wide rows (a whole query: 128 x 136 floats = 69 632 B): one workgroup moves a 16 KiB piece of ONE row -- the row index is read
// once per workgroup (scalar), every lane streams 4 x 16 B with no per-element division, loads issued before the stores.
constexpr int kGatherPiece = kGatherThreads * 4;      // float4s per workgroup
template <bool kWrap>
__global__ void __launch_bounds__(kGatherThreads)
gather_rows_wide_kernel(const f32x4 *__restrict__ src, const int64_t *__restrict__ idx, int64_t n_rows, int64_t src_rows, int row_f4,
                        int pieces, float fill, f32x4 *__restrict__ dst) {
    for (int64_t b = blockIdx.x; b < n_rows * pieces; b += gridDim.x) {
        const int64_t r = b / pieces;
        const int piece = (int)(b - r * pieces);
        int64_t srow = idx[r];
        if (kWrap && srow < 0) srow += src_rows;
        const bool ok = srow >= 0 && srow < src_rows;
        const f32x4 *sp = src + (ok ? srow : 0) * row_f4;
        f32x4 *dp = dst + r * row_f4;
        const int c0 = piece * kGatherPiece + threadIdx.x;
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k * kGatherThreads < row_f4) v[k] = ok ? __builtin_nontemporal_load(sp + c0 + k * kGatherThreads) : f32x4{fill, fill, fill, fill};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k * kGatherThreads < row_f4) __builtin_nontemporal_store(v[k], dp + c0 + k * kGatherThreads);
    }
}

template <bool kWrap>
__global__ void __launch_bounds__(kGatherThreads)
gather_rows_scalar_kernel(const float *__restrict__ src, const int64_t *__restrict__ idx, int64_t n_rows, int64_t src_rows,
                          int row_f, float fill, float *__restrict__ dst) {
    const int64_t total = n_rows * row_f;
    for (int64_t e = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kGatherThreads) {
        const int64_t r = e / row_f;
        const int c = (int)(e - r * row_f);
        int64_t s = idx[r];
        if (kWrap && s < 0) s += src_rows;
        dst[e] = s >= 0 && s < src_rows ? src[s * row_f + c] : fill;
    }
}

template <bool kWrap>
int launch_gather(const float *src, int64_t src_rows, const int64_t *idx, int64_t n_rows, int64_t row_floats, float fill, float *dst,
                  void *stream) {
    const bool vec = row_floats % 4 == 0 && ((uintptr_t)src & 15u) == 0 && ((uintptr_t)dst & 15u) == 0;
    const int64_t total = vec ? n_rows * (row_floats / 4) : n_rows * row_floats;
    int64_t blocks = (total + kGatherThreads - 1) / kGatherThreads;
    if (blocks > 256 * 32) blocks = 256 * 32;                      // 32 workgroups per CU, grid-stride beyond
    if (vec && row_floats / 4 >= kGatherPiece / 2) {
        const int row_f4 = (int)(row_floats / 4), pieces = (row_f4 + kGatherPiece - 1) / kGatherPiece;
        int64_t wg = n_rows * pieces;
        if (wg > 256 * 64) wg = 256 * 64;
        hipLaunchKernelGGL(gather_rows_wide_kernel<kWrap>, dim3((unsigned)wg), dim3(kGatherThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const f32x4 *>(src), idx, n_rows, src_rows, row_f4, pieces, fill, reinterpret_cast<f32x4 *>(dst));
    } else if (vec)
        hipLaunchKernelGGL(gather_rows_kernel<kWrap>, dim3((unsigned)blocks), dim3(kGatherThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const f32x4 *>(src), idx, n_rows, src_rows, (int)(row_floats / 4), fill,
                           reinterpret_cast<f32x4 *>(dst));
    else
        hipLaunchKernelGGL(gather_rows_scalar_kernel<kWrap>, dim3((unsigned)blocks), dim3(kGatherThreads), 0, (hipStream_t)stream, src,
                           idx, n_rows, src_rows, (int)row_floats, fill, dst);
    return ltr::launch_status();
}

// dst[rows[r]][:] = src[r][:] for 0 <= rows[r] < dst_rows (T = f32x4 or float, rows of `row` T); the other dst rows are not touched.
// The caller's rows name no destination twice, so plain stores do.
template <class T>
__global__ void __launch_bounds__(kGatherThreads)
scatter_rows_kernel(const T *__restrict__ src, const int64_t *__restrict__ rows, int64_t n_slots, int row, int64_t dst_rows,
                    T *__restrict__ dst) {
    const int64_t total = n_slots * row;
    for (int64_t e = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kGatherThreads) {
        const int64_t r = e / row;
        const int c = (int)(e - r * row);
        const int64_t d = rows[r];
        if (d >= 0 && d < dst_rows) dst[d * row + c] = __builtin_nontemporal_load(src + e);
    }
}

// ------------------------------------------------------------------------------------------ fixed-length slates
// One 256-thread workgroup per listed query.  slate_select decides which k = min(len, S) documents the query keeps and in which slot
// each sits (ascending document order); the two kernels below write the row map / mask from it, the build kernel also the rows.
constexpr int kSlateThreads = 256;

__device__ __forceinline__ uint64_t slate_key(uint64_t seed, uint64_t q, uint64_t j) {
    uint64_t z = seed ^ (q * 0xD1B54A32D192ED03ull + j * 0x9E3779B97F4A7C15ull + 0x8CB92BA72F3D8DD7ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct SlatePick {
    int64_t off;      // the query's first row
    int k;            // real slots (0: the length is outside 1 .. LTR_MAX_SLATE)
    bool direct;      // slot s holds local document s; otherwise slot_doc[s] (SlateLds)
    __device__ __forceinline__ int doc(const int *slot_doc, int slot) const { return direct ? slot : slot_doc[slot]; }
};

// The workgroup's LDS.  keys: after the ranking reused as slot_doc int [S]; kept: 1 = the document's rank is below S.
struct SlateLds {
    uint64_t keys[LTR_MAX_SLATE];
    uint8_t kept[LTR_MAX_SLATE];
    int wave_tot[kSlateThreads / LTR_WAVE];
    __device__ __forceinline__ const int *slot_doc() const { return reinterpret_cast<const int *>(keys); }
};

// Every branch around a barrier is workgroup-uniform (q, off and len are scalars).  Sampling ranks every document by counting over all
// keys, ties by index: rank(j) = #{o : key[o] < key[j] or (key[o] == key[j] and o < j)}, kept when rank < S.  A wave ranks 64
// CONSECUTIVE documents J0 .. J0 + 63 at a time, so the index rule is wave-uniform outside that band: before it one compare per key
// (key[j] < key[o] is what does NOT count), behind it one compare (key[o] < key[j]), the full rule only on the band's 64 keys.  key[o] is
// one LDS address per wave, a broadcast read.  Then each thread counts the kept flags of `chunk` consecutive documents and an exclusive
// scan over the threads gives its first slot: kept documents fill the slots in ascending document order.
__device__ __forceinline__ SlatePick slate_select(const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, long long i,
                                                  int S, int mode, uint64_t seed, SlateLds &lds) {
    const long long q = ltr_wave_uniform(queries ? (long long)queries[i] : i);
    SlatePick p;
    p.off = ltr_wave_uniform(offsets[q]);
    const int64_t len64 = ltr_wave_uniform(offsets[q + 1]) - p.off;
    p.direct = true;
    if (len64 < 1 || len64 > LTR_MAX_SLATE) {
        p.k = 0;
        return p;
    }
    const int len = (int)len64;
    p.k = len < S ? len : S;
    if (mode == LTR_SLATES_FIRST || len <= S) return p;
    p.direct = false;
    const int tid = threadIdx.x, lane = tid & (LTR_WAVE - 1);
    const uint64_t *keys = lds.keys;
    for (int j = tid; j < len; j += kSlateThreads) lds.keys[j] = slate_key(seed, (uint64_t)q, (uint64_t)j);
    __syncthreads();
    for (int J0 = __builtin_amdgcn_readfirstlane(tid - lane); J0 < len; J0 += kSlateThreads) {
        const int j = J0 + lane, J1 = J0 + LTR_WAVE < len ? J0 + LTR_WAVE : len;
        const uint64_t kj = keys[j < len ? j : len - 1];
        int not_below = 0, below = 0;
#pragma unroll 8
        for (int o = 0; o < J0; ++o) not_below += kj < keys[o];
        for (int o = J0; o < J1; ++o) below += (keys[o] < kj) | ((keys[o] == kj) & (o < j));
#pragma unroll 8
        for (int o = J1; o < len; ++o) below += keys[o] < kj;
        if (j < len) lds.kept[j] = J0 - not_below + below < S;
    }
    __syncthreads();                                                   // flags complete, and every thread is done with the keys
    const int chunk = (len + kSlateThreads - 1) / kSlateThreads;       // 1 .. 8 consecutive documents per thread
    const int j0 = tid * chunk, j1 = j0 + chunk < len ? j0 + chunk : len;
    int mine = 0;
    for (int j = j0; j < j1; ++j) mine += lds.kept[j];
    int incl = mine;
    for (int o = 1; o < LTR_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o, LTR_WAVE);
        if (lane >= o) incl += v;
    }
    if (lane == LTR_WAVE - 1) lds.wave_tot[tid / LTR_WAVE] = incl;
    __syncthreads();
    int slot = incl - mine;
    for (int w = 0; w < tid / LTR_WAVE; ++w) slot += lds.wave_tot[w];
    int *slot_doc = reinterpret_cast<int *>(lds.keys);
    for (int j = j0; j < j1; ++j)
        if (lds.kept[j]) slot_doc[slot++] = j;                         // the ranks are a permutation: exactly S kept, slot < S
    __syncthreads();
    return p;
}

// rows / mask (either may be NULL) of listed query i, from the pick
__device__ __forceinline__ void slate_write_map(const SlatePick &p, const int *slot_doc, long long i, int S, int64_t *__restrict__ rows,
                                                uint8_t *__restrict__ mask) {
    for (int s = threadIdx.x; s < S; s += kSlateThreads) {
        const bool real = s < p.k;
        if (rows) rows[i * S + s] = real ? p.off + p.doc(slot_doc, s) : -1;
        if (mask) mask[i * S + s] = real ? 0 : 1;
    }
}

__global__ void __launch_bounds__(kSlateThreads)
slates_select_kernel(const int64_t *__restrict__ offsets, const int32_t *__restrict__ queries, int n_queries, int S, int mode,
                     uint64_t seed, int64_t *__restrict__ rows, uint8_t *__restrict__ mask) {
    __shared__ SlateLds lds;
    const long long i = ltr_block_id();
    if (i >= n_queries) return;
    const SlatePick p = slate_select(offsets, queries, i, S, mode, seed, lds);
    slate_write_map(p, lds.slot_doc(), i, S, rows, mask);
}

// The selection and the copies in one launch (T = f32x4 or float, X rows of `row` T).  The workgroup sweeps its slate's S x row
// elements flat -- lane-contiguous on the output side, row-contiguous pieces on the input side -- four loads in flight per lane
// before the four stores; (slot, column) advance by 256 elements without a division.
template <class T>
__global__ void __launch_bounds__(kSlateThreads)
slates_build_kernel(const T *__restrict__ X, const float *__restrict__ y, const int64_t *__restrict__ offsets,
                    const int32_t *__restrict__ queries, int n_queries, int S, unsigned row, int mode, uint64_t seed, float pad,
                    T *__restrict__ X_out, float *__restrict__ y_out, uint8_t *__restrict__ mask, int64_t *__restrict__ rows) {
    __shared__ SlateLds lds;
    const long long i = ltr_block_id();
    if (i >= n_queries) return;
    const SlatePick p = slate_select(offsets, queries, i, S, mode, seed, lds);
    const int *slot_doc = lds.slot_doc();
    slate_write_map(p, slot_doc, i, S, rows, mask);
    for (int s = threadIdx.x; s < S; s += kSlateThreads) y_out[i * S + s] = s < p.k ? y[p.off + p.doc(slot_doc, s)] : pad;
    const T *src = X + p.off * row;
    T *out = X_out + i * S * row;
    const T zero = {};
    const unsigned total = (unsigned)S * row, step_slot = kSlateThreads / row, step_col = kSlateThreads % row;   // total <= 2^31
    unsigned slot = threadIdx.x / row, col = threadIdx.x % row;
    for (unsigned e = threadIdx.x; e < total; e += 4 * kSlateThreads) {
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (e + u * kSlateThreads < total)
                v[u] = (int)slot < p.k ? __builtin_nontemporal_load(src + (int64_t)p.doc(slot_doc, (int)slot) * row + col) : zero;
            slot += step_slot;
            col += step_col;
            if (col >= row) {
                col -= row;
                ++slot;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e + u * kSlateThreads < total) out[e + u * kSlateThreads] = v[u];
    }
}

// ------------------------------------------------------------------------------------------ svmlight parser
struct Mapped {
    const char *p = nullptr;
    size_t n = 0;
    int fd = -1;
    ~Mapped() {
        if (p && n) munmap(const_cast<char *>(p), n);
        if (fd >= 0) close(fd);
    }
    int open_file(const char *path) {
        fd = open(path, O_RDONLY);
        if (fd < 0) return LTR_ERR_IO;
        struct stat st;
        if (fstat(fd, &st) != 0) return LTR_ERR_IO;
        n = (size_t)st.st_size;
        if (n == 0) return LTR_OK;
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            n = 0;
            return LTR_ERR_IO;
        }
        p = static_cast<const char *>(m);
        return LTR_OK;
    }
};

// byte ranges [b, e) of `parts` chunks, each starting at the beginning of a line
std::vector<std::pair<size_t, size_t>> split_lines(const Mapped &m, int parts) {
    std::vector<std::pair<size_t, size_t>> out;
    size_t b = 0;
    for (int k = 1; k <= parts && b < m.n; ++k) {
        size_t e = k == parts ? m.n : std::max(b, m.n / (size_t)parts * (size_t)k);
        if (e > 0 && e < m.n) {      // move to the first line start at or after e
            const void *nl = memchr(m.p + e - 1, '\n', m.n - (e - 1));
            e = nl ? (size_t)(static_cast<const char *>(nl) - m.p) + 1 : m.n;
        }
        if (e > b) out.emplace_back(b, e);
        b = e;
    }
    return out;
}

inline bool blank_or_comment(const char *s, const char *e) {
    while (s < e && (*s == ' ' || *s == '\t' || *s == '\r')) ++s;
    return s >= e || *s == '#';
}

struct ScanResult {
    int64_t docs = 0;
    int32_t min_fid = 0x7fffffff, max_fid = -1;
    int err = 0;
};

// Bounded numeric parsing: the mapping is NOT NUL-terminated and strtod/strtol skip '\n' as white space, so every token
// is delimited first ([s, t): up to the next blank / '#' / ':' / line end e), copied into a NUL-terminated stack buffer
// and must be consumed ENTIRELY by the conversion.  Empty values ("2:" at a line end), over-long tokens and non-finite
// values (nan, inf, 1e400) are parse errors, as is anything that would read past the line.
inline const char *token_end(const char *s, const char *e, bool stop_at_colon) {
    while (s < e && *s != ' ' && *s != '\t' && *s != '\r' && *s != '\n' && *s != '#' && !(stop_at_colon && *s == ':')) ++s;
    return s;
}

inline bool parse_f64(const char *s, const char *t, double *out) {
    char buf[64];
    const size_t n = (size_t)(t - s);
    if (n == 0 || n >= sizeof(buf)) return false;
    memcpy(buf, s, n);
    buf[n] = 0;
    char *q = nullptr;
    const double v = strtod(buf, &q);
    if (q != buf + n || !(v - v == 0.0)) return false;        // whole token consumed; finite
    if (buf[0] == ' ' || buf[0] == '\t') return false;
    *out = v;
    return true;
}

inline bool parse_i64(const char *s, const char *t, long long *out) {
    if (s >= t || t - s > 19) return false;
    bool neg = false;
    if (*s == '-' || *s == '+') {
        neg = *s == '-';
        if (++s >= t) return false;
    }
    long long v = 0;
    for (; s < t; ++s) {
        if (*s < '0' || *s > '9') return false;
        const int dgt = *s - '0';
        if (v > (0x7fffffffffffffffLL - dgt) / 10) return false;      // 19-digit tokens can pass LLONG_MAX: reject, never overflow
        v = v * 10 + dgt;
    }
    *out = neg ? -v : v;
    return true;
}

// Parse one line [s, e) (e = the '\n' or the end of the mapping; never dereferenced).  X == nullptr: scan only
// (feature-id range).  Returns 0, or LTR_ERR_PARSE.
inline int parse_line(const char *s, const char *e, int n_features, int fid_base, float *X, double *y, int64_t *qid,
                      int32_t *min_fid, int32_t *max_fid) {
    while (s < e && (*s == ' ' || *s == '\t')) ++s;
    const char *t = token_end(s, e, false);
    double label;
    if (!parse_f64(s, t, &label)) return LTR_ERR_PARSE;
    if (y) *y = label;
    s = t;
    if (qid) *qid = -1;
    while (s < e) {
        while (s < e && (*s == ' ' || *s == '\t' || *s == '\r')) ++s;
        if (s >= e || *s == '#') break;
        if (e - s > 4 && s[0] == 'q' && s[1] == 'i' && s[2] == 'd' && s[3] == ':') {
            t = token_end(s + 4, e, false);
            long long v;
            if (!parse_i64(s + 4, t, &v)) return LTR_ERR_PARSE;
            if (qid) *qid = (int64_t)v;
            s = t;
            continue;
        }
        t = token_end(s, e, true);
        long long fid;
        if (t >= e || *t != ':' || !parse_i64(s, t, &fid)) return LTR_ERR_PARSE;
        s = t + 1;
        t = token_end(s, e, false);
        double v;
        if (!parse_f64(s, t, &v)) return LTR_ERR_PARSE;           // "k:" with nothing behind it is an error, like sklearn
        s = t;
        if (fid < 0 || fid > 0x7ffffff0) return LTR_ERR_PARSE;
        if (min_fid && (int32_t)fid < *min_fid) *min_fid = (int32_t)fid;
        if (max_fid && (int32_t)fid > *max_fid) *max_fid = (int32_t)fid;
        if (X) {
            const long long c = fid - fid_base;
            if (c < 0 || c >= n_features) return LTR_ERR_PARSE;
            X[c] = (float)v;                     // float64 parse, then the reference's astype(np.float32) (dataset.py:63)
        }
    }
    return 0;
}

template <class F>
int for_each_line(const char *b, const char *e, F f) {
    while (b < e) {
        const char *nl = static_cast<const char *>(memchr(b, '\n', (size_t)(e - b)));
        const char *le = nl ? nl : e;
        if (!blank_or_comment(b, le))
            if (int rc = f(b, le)) return rc;
        b = nl ? nl + 1 : e;
    }
    return 0;
}

int clamp_threads(int n) {
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    return n < 1 ? 1 : (n > 64 ? 64 : n);
}

}  // namespace

extern "C" {

int ltr_gather_rows_f32(const float *src, int64_t src_rows, const int64_t *idx, int64_t n_rows, int64_t row_floats,
                        float *dst, void *stream) {
    if (!src || !idx || !dst) return LTR_ERR_NULL;
    if (n_rows < 0 || src_rows < 0 || row_floats < 1 || row_floats > (1 << 28)) return LTR_ERR_SHAPE;
    if (n_rows == 0) return LTR_OK;
    return launch_gather<true>(src, src_rows, idx, n_rows, row_floats, 0.f, dst, stream);
}

int ltr_slates_select(const int64_t *offsets, const int32_t *queries, int n_queries, int S, int mode, uint64_t seed, int64_t *rows,
                      uint8_t *mask, void *stream) {
    if (!offsets || !rows) return LTR_ERR_NULL;
    if (n_queries < 0 || S < 1 || S > LTR_MAX_SLATE) return LTR_ERR_SHAPE;
    if (mode != LTR_SLATES_FIRST && mode != LTR_SLATES_SAMPLE) return LTR_ERR_PARAM;
    if (n_queries == 0) return LTR_OK;
    hipLaunchKernelGGL(slates_select_kernel, ltr_grid(n_queries), dim3(kSlateThreads), 0, (hipStream_t)stream, offsets, queries,
                       n_queries, S, mode, seed, rows, mask);
    return ltr::launch_status();
}

int ltr_slates_gather_f32(const float *src, int64_t src_rows, const int64_t *rows, int64_t n_slots, int64_t row_floats, float fill,
                          float *dst, void *stream) {
    if (!src || !rows || !dst) return LTR_ERR_NULL;
    if (n_slots < 0 || src_rows < 0 || row_floats < 1 || row_floats > (1 << 28)) return LTR_ERR_SHAPE;
    if (n_slots == 0) return LTR_OK;
    return launch_gather<false>(src, src_rows, rows, n_slots, row_floats, fill, dst, stream);
}

int ltr_slates_scatter_f32(const float *src, const int64_t *rows, int64_t n_slots, int64_t row_floats, int64_t dst_rows, float *dst,
                           void *stream) {
    if (!src || !rows || !dst) return LTR_ERR_NULL;
    if (n_slots < 0 || dst_rows < 0 || row_floats < 1 || row_floats > (1 << 28)) return LTR_ERR_SHAPE;
    if (n_slots == 0) return LTR_OK;
    const bool vec = row_floats % 4 == 0 && ((uintptr_t)src & 15u) == 0 && ((uintptr_t)dst & 15u) == 0;
    const int row = (int)(vec ? row_floats / 4 : row_floats);
    int64_t blocks = (n_slots * row + kGatherThreads - 1) / kGatherThreads;
    if (blocks > 256 * 32) blocks = 256 * 32;                      // grid-stride beyond, as the gather
    if (vec)
        hipLaunchKernelGGL(scatter_rows_kernel<f32x4>, dim3((unsigned)blocks), dim3(kGatherThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const f32x4 *>(src), rows, n_slots, row, dst_rows, reinterpret_cast<f32x4 *>(dst));
    else
        hipLaunchKernelGGL(scatter_rows_kernel<float>, dim3((unsigned)blocks), dim3(kGatherThreads), 0, (hipStream_t)stream, src, rows,
                           n_slots, row, dst_rows, dst);
    return ltr::launch_status();
}

int ltr_slates_build(const float *X, const float *y, const int64_t *offsets, const int32_t *queries, int n_queries, int S, int F,
                     int mode, uint64_t seed, float pad, float *X_out, float *y_out, uint8_t *mask, int64_t *rows, void *stream) {
    if (!X || !y || !offsets || !X_out || !y_out) return LTR_ERR_NULL;
    if (n_queries < 0 || S < 1 || S > LTR_MAX_SLATE || F < 1 || F > (1 << 20)) return LTR_ERR_SHAPE;
    if (mode != LTR_SLATES_FIRST && mode != LTR_SLATES_SAMPLE) return LTR_ERR_PARAM;
    if (n_queries == 0) return LTR_OK;
    if (F % 4 == 0 && ((uintptr_t)X & 15u) == 0 && ((uintptr_t)X_out & 15u) == 0)
        hipLaunchKernelGGL(slates_build_kernel<f32x4>, ltr_grid(n_queries), dim3(kSlateThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const f32x4 *>(X), y, offsets, queries, n_queries, S, (unsigned)(F / 4), mode, seed, pad,
                           reinterpret_cast<f32x4 *>(X_out), y_out, mask, rows);
    else
        hipLaunchKernelGGL(slates_build_kernel<float>, ltr_grid(n_queries), dim3(kSlateThreads), 0, (hipStream_t)stream, X, y, offsets,
                           queries, n_queries, S, (unsigned)F, mode, seed, pad, X_out, y_out, mask, rows);
    return ltr::launch_status();
}

int ltr_svmlight_scan(const char *path, int64_t *n_docs, int32_t *min_feature_id, int32_t *max_feature_id, int n_threads) {
    if (!path || !n_docs || !min_feature_id || !max_feature_id) return LTR_ERR_NULL;
    Mapped m;
    if (int rc = m.open_file(path)) return rc;
    const auto parts = split_lines(m, clamp_threads(n_threads));
    std::vector<ScanResult> res(parts.size());
    std::vector<std::thread> th;
    for (size_t t = 0; t < parts.size(); ++t)
        th.emplace_back([&, t] {
            ScanResult &r = res[t];
            r.err = for_each_line(m.p + parts[t].first, m.p + parts[t].second, [&](const char *b, const char *e) {
                ++r.docs;
                return parse_line(b, e, 0, 0, nullptr, nullptr, nullptr, &r.min_fid, &r.max_fid);
            });
        });
    for (auto &t : th) t.join();
    int64_t docs = 0;
    int32_t lo = 0x7fffffff, hi = -1;
    for (const auto &r : res) {
        if (r.err) return r.err;
        docs += r.docs;
        lo = std::min(lo, r.min_fid);
        hi = std::max(hi, r.max_fid);
    }
    *n_docs = docs;
    *min_feature_id = hi < 0 ? 0 : lo;
    *max_feature_id = hi;
    return LTR_OK;
}

int ltr_svmlight_load(const char *path, int64_t n_docs, int n_features, int feature_id_base, float *X, double *y,
                      int64_t *qid, int n_threads) {
    if (!path || !X || !y || !qid) return LTR_ERR_NULL;
    if (n_docs < 0 || n_features < 1) return LTR_ERR_SHAPE;
    Mapped m;
    if (int rc = m.open_file(path)) return rc;
    const auto parts = split_lines(m, clamp_threads(n_threads));
    // pass 1: lines per chunk -> row offsets
    std::vector<int64_t> count(parts.size(), 0);
    {
        std::vector<std::thread> th;
        for (size_t t = 0; t < parts.size(); ++t)
            th.emplace_back([&, t] {
                for_each_line(m.p + parts[t].first, m.p + parts[t].second, [&](const char *, const char *) {
                    ++count[t];
                    return 0;
                });
            });
        for (auto &t : th) t.join();
    }
    std::vector<int64_t> first(parts.size() + 1, 0);
    for (size_t t = 0; t < parts.size(); ++t) first[t + 1] = first[t] + count[t];
    if (first[parts.size()] != n_docs) return LTR_ERR_SHAPE;
    std::vector<int> err(parts.size(), 0);
    std::vector<std::thread> th;
    for (size_t t = 0; t < parts.size(); ++t)
        th.emplace_back([&, t] {
            int64_t row = first[t];
            err[t] = for_each_line(m.p + parts[t].first, m.p + parts[t].second, [&](const char *b, const char *e) {
                float *xr = X + (size_t)row * n_features;
                memset(xr, 0, sizeof(float) * (size_t)n_features);                   // absent features are 0 (sparse format)
                const int rc = parse_line(b, e, n_features, feature_id_base, xr, y + row, qid + row, nullptr, nullptr);
                ++row;
                return rc;
            });
        });
    for (auto &t : th) t.join();
    for (int e : err)
        if (e) return e;
    return LTR_OK;
}

}  // extern "C"
