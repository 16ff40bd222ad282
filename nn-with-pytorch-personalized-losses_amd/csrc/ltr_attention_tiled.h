// ltr_attention_tiled.h -- key-tiled attention for slates of 513..2048 documents (included by ltr_encoder.hip inside its
// anonymous namespace, after the whole-row attention kernels whose helpers it reuses: AttArgs, load8, store4, row_frag,
// col_frag, quad_sum / quad_max, dot8, the dropout stream and attn_idx).
//
// The whole-row kernels hold one (slate, head) in one workgroup and a 16-query tile's whole score row in registers, which
// bounds them at S = 512.  Here the work is split by query block (forward, dQ) or key block (dK / dV) and the other axis is
// walked in 64-token tiles staged in LDS:
//   * forward: one workgroup per (slate, head, 64-query block), 4 waves x 16 queries, online softmax in the base-2 form of
//     softmax_tile (c2 = log2(e) / sqrt(dk) in the exponent, -inf bias for masked keys): running max m and sum l per query,
//     O rescaled by 2^(m_old - m_new) when the max grows.  Dropout multiplies the UNNORMALISED p~ before the P V MFMA; l sums the
//     un-dropped p~; the epilogue scales O by (1/(1-p)) / l.  lse2 = m + log2 l (+inf for a query without an unmasked key).
//   * backward, two launches on the caller's stream, each output element written by exactly one lane (no atomics, no scratch):
//       dK / dV: one workgroup per (slate, head, 64-key block), key on lane & 15 (the S orientation of the whole-row kernel's
//                phase B), query tiles of 64 staged with their lse2 and D_q = dctx_q . ctx_q;
//       dQ:      one workgroup per (slate, head, 64-query block), the S^T orientation of phase A, key tiles of 64 staged.
//     Both recompute p = 2^(c2 s - lse2) from the forward's lse2 and the same keep mask.
//   * staging (guide T14): the next tile's global loads are issued into registers before the current tile's MFMAs and written
//     to LDS after the next barrier.
// Dropout indices are the whole-row kernels' (attn_idx with Sp = S rounded up to 32), so ltr_enc_attn_dropout_mask exports the
// masks of these kernels too.

constexpr int kTile = 64;                                  // tokens per staged tile = queries per block = keys per block
constexpr int kTileLd = ((kTile / 2 + 59) / 64 * 64 + 4) * 2;   // tr_ld(64): [d][token] image row stride
constexpr int kTiledMaxS = 2048;

// workgroup id -> (slate, head, block), the XCD-aware mapping of att_slate_head extended by the block index: every block of
// every head of slate b gets an id of residue class b mod 8, i.e. one XCD and one L2 per slate.
__device__ __forceinline__ bool att_tiled_ids(int B, int h, int nblk, int &b, int &hd, int &blk) {
    const int x = blockIdx.x & 7, n = blockIdx.x >> 3, per = h * nblk;
    b = (n / per) * 8 + x;
    hd = (n % per) / nblk;
    blk = n % nblk;
    return b < B;
}
inline unsigned att_tiled_grid(int B, int h, int S) { return (unsigned)((B + 7) / 8 * 8 * h * ((S + kTile - 1) / kTile)); }

// base of head hd of slate b in source `which` (0 Q, 1 K, 2 V of qkv; 3 dctx; 4 ctx) and its token stride
__device__ __forceinline__ const bf16_t *att_head_base(const AttArgs &a, int b, int hd, int which, long long &ld) {
    const int d = a.h * a.dk;
    ld = which < 3 ? 3 * d : d;
    const bf16_t *p = which < 3 ? a.qkv + which * d : (which == 3 ? a.dctx : a.ctx);
    return p + (long long)b * a.S * ld + hd * a.dk;
}
// thread tid's share of a 64-token tile: token tid >> 2, features 8 (tid & 3) .. +7
__device__ __forceinline__ u32x4 tile_load(const bf16_t *base, long long ld, int t0, int dk, bool vec, int S) {
    const int tok = t0 + (threadIdx.x >> 2);
    return load8(base + (long long)tok * ld, 8 * (threadIdx.x & 3), dk, vec, tok < S);
}
__device__ __forceinline__ void tile_store(bf16_t *rows, bf16_t *tr, const u32x4 &v) {
    const int tok = threadIdx.x >> 2, ch = threadIdx.x & 3;
    if (rows) *reinterpret_cast<u32x4 *>(rows + tok * kRowLd + 8 * ch) = v;
    if (tr) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            tr[(8 * ch + 2 * x) * kTileLd + tok] = (bf16_t)(v[x] & 0xffffu);
            tr[(8 * ch + 2 * x + 1) * kTileLd + tok] = (bf16_t)(v[x] >> 16);
        }
    }
}
__device__ __forceinline__ float key_bias(const AttArgs &a, int b, int k) {
    return k >= a.S || (a.mask && a.mask[(long long)b * a.S + k] == 1) ? -INFINITY : 0.f;
}

__global__ void __launch_bounds__(kAttThreads) attention_fwd_tiled_kernel(AttArgs a) {
    static_assert(kAttThreads == 4 * kTile, "one 8-feature chunk of one tile token per thread");
    __shared__ __attribute__((aligned(16))) bf16_t Kimg[kTile * kRowLd];
    __shared__ __attribute__((aligned(16))) bf16_t VT[kDkPad * kTileLd];
    __shared__ __attribute__((aligned(16))) float biasT[kTile];
    const int nqb = (a.S + kTile - 1) / kTile;
    int b, hd, qb;
    if (!att_tiled_ids(a.B, a.h, nqb, b, hd, qb)) return;
    const int d = a.h * a.dk, bh = b * a.h + hd, Sp = round_up(a.S, 32);
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool vec = a.dk % 8 == 0;
    const float c2 = 1.44269504088896341f / sqrtf((float)a.dk);
    const unsigned thr = drop_threshold(a.drop_p);
    const float ks = thr ? 1.f / (1.f - a.drop_p) : 1.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    long long ldk, ldv;
    const bf16_t *kbase = att_head_base(a, b, hd, 1, ldk), *vbase = att_head_base(a, b, hd, 2, ldv);

    const int q0 = qb * kTile + 16 * w, query = q0 + j;
    const bool active = q0 < a.S;                               // wave-uniform; idle waves still take part in the barriers
    const u32x4 qf = load8(a.qkv + ((long long)b * a.S + query) * 3 * d + hd * a.dk, 8 * g, a.dk, vec, query < a.S);
    float m = -INFINITY, l = 0.f;                               // running max (quad-uniform) and this lane's share of the sum
    f32x4 o[2] = {zero, zero};

    const int nkt = (a.S + kTile - 1) / kTile;
    u32x4 kreg = tile_load(kbase, ldk, 0, a.dk, vec, a.S), vreg = tile_load(vbase, ldv, 0, a.dk, vec, a.S);
    float breg = threadIdx.x < kTile ? key_bias(a, b, threadIdx.x) : 0.f;
    for (int t = 0; t < nkt; ++t) {
        const int k0 = t * kTile;
        __syncthreads();                                        // the previous tile's readers are done
        tile_store(Kimg, nullptr, kreg);
        tile_store(nullptr, VT, vreg);
        if (threadIdx.x < kTile) biasT[threadIdx.x] = breg;
        __syncthreads();
        if (t + 1 < nkt) {                                      // issue the next tile's loads under this tile's math
            kreg = tile_load(kbase, ldk, k0 + kTile, a.dk, vec, a.S);
            vreg = tile_load(vbase, ldv, k0 + kTile, a.dk, vec, a.S);
            if (threadIdx.x < kTile) breg = key_bias(a, b, k0 + kTile + threadIdx.x);
        }
        if (!active) continue;
        f32x4 st[4];
        float mt = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            st[kt] = mfma_bf16(row_frag(Kimg, kt, lane), qf, zero);      // S^T[key k0 + 16 kt + 4 g + r][query]
            const f32x4 bias = *reinterpret_cast<const f32x4 *>(biasT + 16 * kt + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                st[kt][r] = fmaf(st[kt][r], c2, bias[r]);
                mt = fmaxf(mt, st[kt][r]);
            }
        }
        mt = quad_max(mt);
        const float mn = fmaxf(m, mt), mu = mn == -INFINITY ? 0.f : mn;
        if (mn != m) {                                          // the row max grew: rescale what was summed at the old one
            const float alpha = __builtin_amdgcn_exp2f(m - mu);   // m = -inf: nothing summed yet, alpha = 0
            l *= alpha;
            o[0] *= alpha;
            o[1] *= alpha;
            m = mn;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            unsigned pk[4];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f32x4 p;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = __builtin_amdgcn_exp2f(st[2 * u + half][r] - mu);
                    l += p[r];
                }
                if (thr) {
                    const Keep4 keep = drop_keep4b(a.seed, a.stream_id, attn_idx(bh, Sp, query, k0 + 32 * u + 16 * half + 4 * g), thr);
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[r] = keep.k[r] ? p[r] : 0.f;
                }
                pk[2 * half] = pack_bf16(p[0], p[1]);
                pk[2 * half + 1] = pack_bf16(p[2], p[3]);
            }
            const u32x4 pf = {pk[0], pk[1], pk[2], pk[3]};
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[dt] = mfma_bf16(col_frag(VT, kTileLd, dt, u, lane), pf, o[dt]);
        }
    }
    if (!active) return;
    l = quad_sum(l);
    const float inv = l > 0.f ? ks / l : 0.f;
    if (a.lse && g == 0 && query < a.S) a.lse[(long long)bh * a.S + query] = l > 0.f ? m + __builtin_amdgcn_logf(l) : INFINITY;
    if (query < a.S) {
        bf16_t *row = a.out + ((long long)b * a.S + query) * d + hd * a.dk;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) store4(row, 16 * dt + 4 * g, a.dk, a.dk % 4 == 0, o[dt] * inv);
    }
}

// dK / dV: key on lane & 15 of wave w (keys kb*64 + 16 w ..), query tiles of 64 staged as Q / dO rows and Q^T / dO^T images with
// their lse2 (+inf for padded queries: p = 0) and D_q = dO_q . O_q (0 for padded queries).
__global__ void __launch_bounds__(kAttThreads) attention_bwd_kv_tiled_kernel(AttArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Qr[kTile * kRowLd];
    __shared__ __attribute__((aligned(16))) bf16_t dOr[kTile * kRowLd];
    __shared__ __attribute__((aligned(16))) bf16_t QT[kDkPad * kTileLd];
    __shared__ __attribute__((aligned(16))) bf16_t dOT[kDkPad * kTileLd];
    __shared__ __attribute__((aligned(16))) float lseS[kTile];
    __shared__ __attribute__((aligned(16))) float DS[kTile];
    const int nkb = (a.S + kTile - 1) / kTile;
    int b, hd, kb;
    if (!att_tiled_ids(a.B, a.h, nkb, b, hd, kb)) return;
    const int d = a.h * a.dk, bh = b * a.h + hd, Sp = round_up(a.S, 32);
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool vec = a.dk % 8 == 0;
    const float scale = 1.f / sqrtf((float)a.dk), c2 = 1.44269504088896341f * scale;
    const unsigned thr = drop_threshold(a.drop_p);
    const float ks = thr ? 1.f / (1.f - a.drop_p) : 1.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    long long ldq, ldo, ldc;
    const bf16_t *qbase = att_head_base(a, b, hd, 0, ldq), *obase = att_head_base(a, b, hd, 3, ldo), *cbase = att_head_base(a, b, hd, 4, ldc);
    const float *lse_bh = a.lse + (long long)bh * a.S;

    const int k0w = kb * kTile + 16 * w, key = k0w + j;
    const bool active = k0w < a.S;
    const long long tok = (long long)b * a.S + key;
    const u32x4 kf = load8(a.qkv + tok * 3 * d + d + hd * a.dk, 8 * g, a.dk, vec, key < a.S);
    const u32x4 vf = load8(a.qkv + tok * 3 * d + 2 * d + hd * a.dk, 8 * g, a.dk, vec, key < a.S);
    const bool masked = key_bias(a, b, key) != 0.f;
    f32x4 dv[2] = {zero, zero}, dkk[2] = {zero, zero};

    // thread tid stages token tid >> 2 of the tile; its lane quad (tid & 3) sums D over the four 8-feature chunks
    auto load_d = [&](int q0, const u32x4 &dof) -> float {
        const u32x4 of = tile_load(cbase, ldc, q0, a.dk, vec, a.S);
        float s = dot8(dof, of);
        s += __shfl_xor(s, 1, 64);
        return s + __shfl_xor(s, 2, 64);
    };
    const int nqt = (a.S + kTile - 1) / kTile;
    u32x4 qreg = tile_load(qbase, ldq, 0, a.dk, vec, a.S), oreg = tile_load(obase, ldo, 0, a.dk, vec, a.S);
    float dreg = load_d(0, oreg);
    const int qs = threadIdx.x >> 2;
    float lreg = qs < a.S ? lse_bh[qs] : INFINITY;
    for (int t = 0; t < nqt; ++t) {
        const int q0 = t * kTile;
        __syncthreads();
        tile_store(Qr, QT, qreg);
        tile_store(dOr, dOT, oreg);
        if ((threadIdx.x & 3) == 0) {
            lseS[qs] = lreg;
            DS[qs] = dreg;
        }
        __syncthreads();
        if (t + 1 < nqt) {
            const int q1 = q0 + kTile;
            qreg = tile_load(qbase, ldq, q1, a.dk, vec, a.S);
            oreg = tile_load(obase, ldo, q1, a.dk, vec, a.S);
            dreg = load_d(q1, oreg);
            lreg = q1 + qs < a.S ? lse_bh[q1 + qs] : INFINITY;
        }
        if (!active) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            unsigned pk[4], dk4[4];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int qt = 2 * u + half;
                const f32x4 s = mfma_bf16(row_frag(Qr, qt, lane), kf, zero);       // S[query q0 + 16 qt + 4 g + r][key]
                const f32x4 dpd = mfma_bf16(row_frag(dOr, qt, lane), vf, zero);    // dPd[query][key]
                const f32x4 l4 = *reinterpret_cast<const f32x4 *>(lseS + 16 * qt + 4 * g);
                const f32x4 d4 = *reinterpret_cast<const f32x4 *>(DS + 16 * qt + 4 * g);
                const Keep4 keep4 = thr ? drop_keep_col4b(a.seed, a.stream_id, attn_idx(bh, Sp, q0 + 16 * qt + 4 * g, key),
                                                          (unsigned long long)Sp, thr, lane)
                                        : keep_all();
                f32x4 pd, ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = masked ? 0.f : __builtin_amdgcn_exp2f(s[r] * c2 - l4[r]);
                    const bool keep = keep4.k[r];
                    pd[r] = keep ? p * ks : 0.f;
                    ds[r] = p * ((keep ? dpd[r] * ks : 0.f) - d4[r]) * scale;
                }
                pk[2 * half] = pack_bf16(pd[0], pd[1]);
                pk[2 * half + 1] = pack_bf16(pd[2], pd[3]);
                dk4[2 * half] = pack_bf16(ds[0], ds[1]);
                dk4[2 * half + 1] = pack_bf16(ds[2], ds[3]);
            }
            const u32x4 pf = {pk[0], pk[1], pk[2], pk[3]}, dsf = {dk4[0], dk4[1], dk4[2], dk4[3]};
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                dv[dt] = mfma_bf16(col_frag(dOT, kTileLd, dt, u, lane), pf, dv[dt]);
                dkk[dt] = mfma_bf16(col_frag(QT, kTileLd, dt, u, lane), dsf, dkk[dt]);
            }
        }
    }
    if (active && key < a.S) {
        bf16_t *row = a.out + tok * 3 * d + hd * a.dk;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            store4(row + d, 16 * dt + 4 * g, a.dk, a.dk % 4 == 0, dkk[dt]);
            store4(row + 2 * d, 16 * dt + 4 * g, a.dk, a.dk % 4 == 0, dv[dt]);
        }
    }
}

// dQ: query on lane & 15 of wave w (the forward's orientation), key tiles of 64 staged as K / V rows, K^T and the key bias.
__global__ void __launch_bounds__(kAttThreads) attention_bwd_q_tiled_kernel(AttArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Kr[kTile * kRowLd];
    __shared__ __attribute__((aligned(16))) bf16_t Vr[kTile * kRowLd];
    __shared__ __attribute__((aligned(16))) bf16_t KT[kDkPad * kTileLd];
    __shared__ __attribute__((aligned(16))) float biasT[kTile];
    const int nqb = (a.S + kTile - 1) / kTile;
    int b, hd, qb;
    if (!att_tiled_ids(a.B, a.h, nqb, b, hd, qb)) return;
    const int d = a.h * a.dk, bh = b * a.h + hd, Sp = round_up(a.S, 32);
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool vec = a.dk % 8 == 0;
    const float scale = 1.f / sqrtf((float)a.dk), c2 = 1.44269504088896341f * scale;
    const unsigned thr = drop_threshold(a.drop_p);
    const float ks = thr ? 1.f / (1.f - a.drop_p) : 1.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    long long ldk, ldv;
    const bf16_t *kbase = att_head_base(a, b, hd, 1, ldk), *vbase = att_head_base(a, b, hd, 2, ldv);

    const int q0 = qb * kTile + 16 * w, query = q0 + j;
    const bool active = q0 < a.S, valid = query < a.S;
    const long long tok = (long long)b * a.S + query;
    const u32x4 qf = load8(a.qkv + tok * 3 * d + hd * a.dk, 8 * g, a.dk, vec, valid);
    const u32x4 dof = load8(a.dctx + tok * d + hd * a.dk, 8 * g, a.dk, vec, valid);
    const u32x4 of = load8(a.ctx + tok * d + hd * a.dk, 8 * g, a.dk, vec, valid);
    const float D = quad_sum(dot8(dof, of));
    const float lq = valid ? a.lse[(long long)bh * a.S + query] : INFINITY;
    f32x4 dq[2] = {zero, zero};

    const int nkt = (a.S + kTile - 1) / kTile;
    u32x4 kreg = tile_load(kbase, ldk, 0, a.dk, vec, a.S), vreg = tile_load(vbase, ldv, 0, a.dk, vec, a.S);
    float breg = threadIdx.x < kTile ? key_bias(a, b, threadIdx.x) : 0.f;
    for (int t = 0; t < nkt; ++t) {
        const int k0 = t * kTile;
        __syncthreads();
        tile_store(Kr, KT, kreg);
        tile_store(Vr, nullptr, vreg);
        if (threadIdx.x < kTile) biasT[threadIdx.x] = breg;
        __syncthreads();
        if (t + 1 < nkt) {
            kreg = tile_load(kbase, ldk, k0 + kTile, a.dk, vec, a.S);
            vreg = tile_load(vbase, ldv, k0 + kTile, a.dk, vec, a.S);
            if (threadIdx.x < kTile) breg = key_bias(a, b, k0 + kTile + threadIdx.x);
        }
        if (!active) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            unsigned pk[4];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int kt = 2 * u + half;
                const f32x4 s = mfma_bf16(row_frag(Kr, kt, lane), qf, zero);       // S^T[key k0 + 16 kt + 4 g + r][query]
                const f32x4 dp = mfma_bf16(row_frag(Vr, kt, lane), dof, zero);     // dPd^T = V dO^T
                const f32x4 bias = *reinterpret_cast<const f32x4 *>(biasT + 16 * kt + 4 * g);
                const Keep4 keep = thr ? drop_keep4b(a.seed, a.stream_id, attn_idx(bh, Sp, query, k0 + 16 * kt + 4 * g), thr) : keep_all();
                f32x4 ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, bias[r]) - lq);
                    ds[r] = p * ((keep.k[r] ? dp[r] * ks : 0.f) - D) * scale;
                }
                pk[2 * half] = pack_bf16(ds[0], ds[1]);
                pk[2 * half + 1] = pack_bf16(ds[2], ds[3]);
            }
            const u32x4 dsf = {pk[0], pk[1], pk[2], pk[3]};
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) dq[dt] = mfma_bf16(col_frag(KT, kTileLd, dt, u, lane), dsf, dq[dt]);
        }
    }
    if (active && valid) {
        bf16_t *row = a.out + tok * 3 * d + hd * a.dk;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) store4(row, 16 * dt + 4 * g, a.dk, a.dk % 4 == 0, dq[dt]);
    }
}

// p_attn for any S <= 2048: one wave per (slate-head, query), lanes over keys.  Pass 1: per-lane online max / sum, combined
// over the wave into lse2; pass 2: probs = dropout(2^(c2 s - lse2)).  Not a hot kernel.
__device__ __forceinline__ float probs_score(const AttArgs &a, int b, const bf16_t *qrow, const bf16_t *base, int d, int k, float c2) {
    if (k >= a.S || (a.mask && a.mask[(long long)b * a.S + k] == 1)) return -INFINITY;
    const bf16_t *krow = base + (long long)k * 3 * d + d;
    float acc = 0.f;
    for (int e = 0; e < a.dk; ++e) acc = fmaf(from_bf16(qrow[e]), from_bf16(krow[e]), acc);
    return acc * c2;
}
__global__ void __launch_bounds__(256) attn_probs_tiled_kernel(AttArgs a, float *__restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)a.B * a.h * a.S) return;
    const int query = (int)(row % a.S), bh = (int)(row / a.S), b = bh / a.h, hd = bh % a.h;
    const int d = a.h * a.dk, Sp = round_up(a.S, 32);
    const bf16_t *base = a.qkv + (long long)b * a.S * 3 * d + hd * a.dk;
    const bf16_t *qrow = base + (long long)query * 3 * d;
    const float c2 = 1.44269504088896341f / sqrtf((float)a.dk);
    float m = -INFINITY, l = 0.f;
    for (int k = lane; k < a.S; k += 64) {
        const float v = probs_score(a, b, qrow, base, d, k, c2);
        if (v == -INFINITY) continue;
        if (v > m) {
            l = l * __builtin_amdgcn_exp2f(m - v) + 1.f;
            m = v;
        } else {
            l += __builtin_amdgcn_exp2f(v - m);
        }
    }
    float M = m;
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    l = m == -INFINITY ? 0.f : l * __builtin_amdgcn_exp2f(m - M);
    l = wave_sum(l);
    const float lse2 = l > 0.f ? M + __builtin_amdgcn_logf(l) : INFINITY;
    const unsigned thr = drop_threshold(a.drop_p);
    const float ks = thr ? 1.f / (1.f - a.drop_p) : 1.f;
    for (int k = lane; k < a.S; k += 64) {
        float pv = __builtin_amdgcn_exp2f(probs_score(a, b, qrow, base, d, k, c2) - lse2);
        if (thr) pv = drop_keep(a.seed, a.stream_id, attn_idx(bh, Sp, query, k), thr) ? pv * ks : 0.f;
        probs[row * a.S + k] = pv;
    }
}

inline int launch_att_tiled_fwd(const AttArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(attention_fwd_tiled_kernel, dim3(att_tiled_grid(a.B, a.h, a.S)), dim3(kAttThreads), 0, stream, a);
    return status();
}
// the two backward kernels write disjoint columns of dqkv (dK | dV, then dQ): stream-ordered, no side stream
inline int launch_att_tiled_bwd(const AttArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(attention_bwd_kv_tiled_kernel, dim3(att_tiled_grid(a.B, a.h, a.S)), dim3(kAttThreads), 0, stream, a);
    if (int rc = status()) return rc;
    hipLaunchKernelGGL(attention_bwd_q_tiled_kernel, dim3(att_tiled_grid(a.B, a.h, a.S)), dim3(kAttThreads), 0, stream, a);
    return status();
}
inline int launch_att_probs_tiled(const AttArgs &a, float *probs, hipStream_t stream) {
    const long long rows = (long long)a.B * a.h * a.S;
    hipLaunchKernelGGL(attn_probs_tiled_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a, probs);
    return status();
}
