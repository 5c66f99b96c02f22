// Attention core backward under an ADDITIVE fp32 bias and a head mask, with or without PREFIX rows (CDNA4 / gfx950; head size 64,
// S queries against L = P + S <= 256 keys, P >= 0 prefix keys): the backward of modcr_qkv_attn_bias_fwd's arithmetic
// (modeling_bert.py:55-68 under autograd).  Per (sequence n, head a), keys j < P are the prefix rows (history_state), keys j >= P the
// sequence's own rows (the forward's order):
//     s_ij = q_i.k_j / 8 + bias[n, a, i, j]     P = softmax_j(s)     P' = P o m / (1 - p)     P'' = hm[n, a] P'     ctx = P''.V
//     dV = P''^T.dctx     dP = hm (m / (1 - p)) o (dctx.V^T)     dS = P o (dP - rowsum(dP o P))
//     dQ = dS.K / 8  [S rows]     dK = dS^T.Q / 8  [L rows]     d_bias = dS  [N, A, S, L]
// from the recomputed rows: the own rows' q | k | v projection [N*S][3H] and, with P > 0, the prefix rows' k | v projection
// [N*P][2H].  modcr_qkv_attn_bias_bwd calls with P = 0, modcr_qkv_attn_prefix_bwd with P > 0, modcr_qkv_attn_gate_bwd with either and
// with d_head_mask (DHM: d_hm[n, a] = sum_i dctx_i . (P'.V)_i, the derivative with respect to hm itself); PREFIX = false makes P the
// compile-time constant 0, and every select between the two row buffers and every skip of an empty block falls away.  Both cores
// recompute the row statistics (the bias forward writes none) and follow the older binary cores of attn.hip step for step --
// attn_bias_bwd_mfma_kernel is attn_bwd_mfma_kernel (bf16 rows, L <= 192, two sub-passes, accumulators as operands),
// attn_bias_bwd_f32_kernel is attn_bwd_f32_kernel (fp32 rows, L <= 256).  The conventions:
//   * the score accumulator is initialised from bias[n sn + a sa + q sq + key] x log2e (strides in elements, 0 = broadcast, unit key
//     stride; never expanded) instead of the key mask / mask bits; keys beyond L carry -inf;
//   * the K | V images (pass A: K, V in LDS) hold L rows, the first P from the prefix rows' buffer; the Qs | dO images (pass B: Q, dO
//     in LDS) hold S rows;
//   * the head's multiplier hm is a common factor of dP and so of every result: hm = 0 makes dQ, dK, dV and d_bias exactly 0;
//   * dS leaves as fp32 [N, A, S, L] (d_bias) and dQ for S rows from the sub-pass that owns the QUERIES; dK | dV for L rows leave from
//     the sub-pass that owns the KEYS: the first P to the prefix gradient rows [N*P][2H], the rest to the own rows' dq | dk | dv
//     [N*S][3H].  Every output element is written by exactly one lane, nothing is accumulated across workgroups -- no atomics, two
//     launches are bit-identical;
//   * the dropout mask is the forward's: counter row (n A + a) x 256 + QUERY index (0 .. S - 1), key index over [prefix ; x];
//   * a query row whose every key is -inf: max = -inf is replaced by 0 and 1 / sum = 1 / 0 by 0, so P = 0 on the whole row
//     (the forward's convention) and the row adds exactly nothing to dQ, dK, dV, d_bias.  A single -inf entry is exp2(-inf) = 0.
#include "common.h"
#include "attn_common.h"

namespace {

struct ABB {
    static constexpr int LP = 192, NT = 384;
    static constexpr int ROWS = LP * 128;                   // [token][64] bf16, 128-byte rows, swz128
    static constexpr int IMG = 2 * ROWS;                    // sub-pass Q: K | V    sub-pass K: Qs | dO
    static constexpr int SMEM = IMG + 3 * LP * 4;           // + row max, 1 / row sum, delta
};

// PREFIX: prefix rows are given (else P = 0); BIAS: a bias is given (else the head mask alone); DBIAS: dS leaves as d_bias;
// DHM: the gradient of the head's multiplier leaves as d_head_mask[n A + a].
template <bool PREFIX, bool BIAS, bool DBIAS, bool DHM>
__global__ __launch_bounds__(384, 3) void attn_bias_bwd_mfma_kernel(AttnBiasBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int LP = ABB::LP;
    unsigned char* img0 = smem;                             // rows image 0 (K | Qs)
    unsigned char* img1 = smem + ABB::ROWS;                 // rows image 1 (V | dO)
    float* sM = reinterpret_cast<float*>(smem + ABB::IMG);
    float* sInv = sM + LP;
    float* sDl = sInv + LP;
    const int S = p.S, P = PREFIX ? p.P : 0, L = S + P, H = p.H;
    const int n = blockIdx.x / p.A, a = blockIdx.x % p.A;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15_ = lane & 15, l4_ = lane >> 4;
    const bf16* qkv = reinterpret_cast<const bf16*>(p.qkv) + (int64_t)n * S * 3 * H + a * 64;      // own rows: q | k | v
    const bf16* kvh = reinterpret_cast<const bf16*>(p.kvh) + (int64_t)n * P * 2 * H + a * 64;      // prefix rows: k | v
    const bf16* dctx = reinterpret_cast<const bf16*>(p.dctx) + (int64_t)n * S * H + a * 64;
    const float* bias = BIAS ? p.bias + (int64_t)n * p.bias_sn + (int64_t)a * p.bias_sa : nullptr;
    float* dbias = DBIAS ? p.d_bias + ((int64_t)n * p.A + a) * S * L : nullptr;
    constexpr float QS = 0.125f * LOG2E;
    // The head's multiplier scales dP, hence delta and dS, hence dQ, dK, dV and d_bias, by one factor: the arithmetic below is the
    // binary core's (hm = 1) and hm enters where the results are stored.  (As a factor of every dP element it cost the kernel
    // its third wave per SIMD: 153 -> 168 registers + scratch.)
    const float hm = p.head_mask ? p.head_mask[(int64_t)n * p.head_mask_sn + a] : 1.0f;
    const uint32_t dthr = p.drop_thr16;

    auto zero8 = [] {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)0.f;
        return o;
    };
    // 8 consecutive features of KEY j's k (part 0) or v (part 1) row: prefix rows first, then the own rows; zeros beyond L
    auto kv8 = [&](int j, int part, int c) {
        if (j >= L) return zero8();
        const bf16* row = j < P ? kvh + (int64_t)j * 2 * H + part * H : qkv + (int64_t)(j - P) * 3 * H + (1 + part) * H;
        return *reinterpret_cast<const bf16x8*>(row + c * 8);
    };
    // ... of QUERY i's q row scaled by log2e / 8 and rounded again, or of its dctx row; zeros beyond S
    auto q8 = [&](int i, int c) {
        if (i >= S) return zero8();
        bf16x8 o = *reinterpret_cast<const bf16x8*>(qkv + (int64_t)i * 3 * H + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)o[e] * QS);
        return o;
    };
    auto do8 = [&](int i, int c) { return i < S ? *reinterpret_cast<const bf16x8*>(dctx + (int64_t)i * H + c * 8) : zero8(); };
    auto put_rows = [&](unsigned char* img, int t, int c, const bf16x8& v) { *reinterpret_cast<bf16x8*>(img + swz128(t, c)) = v; };
    // score init (log2 domain) of query q, key: the bias, -inf on a padded key.  A padded query row takes the bias of row S - 1 in
    // both sub-passes: its probabilities are finite and consistent, its dO is zero.  32-bit element offsets inside the (n, a)
    // slice (the host bounds the query stride): one uniform base + a per-lane offset.
    const uint32_t bsq = (uint32_t)p.bias_sq;
    auto init1 = [&](int q, int key) {
        if (key >= L) return -INFINITY;
        if (!BIAS) return 0.f;
        return bias[(uint32_t)min(q, S - 1) * bsq + (uint32_t)key] * LOG2E;
    };

    // ---- the images of sub-pass Q: K | V, L rows --------------------------------------------------------------------
    for (int it = tid; it < LP * 8; it += ABB::NT) {
        const int t = it >> 3, c = it & 7;
        put_rows(img0, t, c, kv8(t, 0, c));
        put_rows(img1, t, c, kv8(t, 1, c));
    }
    __syncthreads();

    const int t0 = wave * 32;                               // this wave's queries (sub-pass Q) / keys (sub-pass K)
    // ---- sub-pass Q: one 16-query block at a time (its 16 x 192 scores = 48 registers).  With prefix rows a wave whose 32 queries
    // all lie beyond S has nothing to do (sub-pass K then reads the statistics of the 32-query tiles below S only) ----------------
#pragma unroll 1
    for (int qb = 0; qb < (PREFIX && t0 >= S ? 0 : 2); ++qb) {
        // per-iteration opaque copies of the lane indices (attn_bwd_mfma_kernel: hoisted fragment addresses were spilled)
        int l15 = l15_, l4 = l4_;
        asm volatile("" : "+v"(l15), "+v"(l4));
        const int qrow = t0 + qb * 16 + l15;
        bf16x8 fq[2], fdo[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            fq[ks] = q8(qrow, ks * 4 + l4);
            fdo[ks] = do8(qrow, ks * 4 + l4);
        }
        // the lane's bias values: query qrow, keys 32 kt + 16 kb + 4 l4 + {0..3}; every load is issued before the first product
        f32x4 sc[6][2];
#pragma unroll
        for (int kt = 0; kt < 6; ++kt)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[kt][kb][e] = init1(qrow, kt * 32 + kb * 16 + 4 * l4 + e);
#pragma unroll
        for (int kt = 0; kt < 6; ++kt)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int krow = kt * 32 + kb * 16;
                const bf16x8 fk0 = *reinterpret_cast<const bf16x8*>(img0 + swz128(krow + l15, l4));
                const bf16x8 fk1 = *reinterpret_cast<const bf16x8*>(img0 + swz128(krow + l15, 4 + l4));
                f32x4 c = sc[kt][kb];
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk0, fq[0], c, 0, 0, 0);
                sc[kt][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk1, fq[1], c, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);          // no hoisting of the next blocks' fragment reads: registers
            }
        {
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 6; ++kt)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) m = fmaxf(m, sc[kt][kb][e]);
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            if (m == -INFINITY) m = 0.f;                    // every key at -inf: exponentials against 0, all of them 0
            float l = 0.f;
#pragma unroll
            for (int kt = 0; kt < 6; ++kt)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float ex = __builtin_amdgcn_exp2f(sc[kt][kb][e] - m); sc[kt][kb][e] = ex; l += ex; }
            l += __shfl_xor(l, 16, 64);
            l += __shfl_xor(l, 32, 64);
            const float inv = l > 0.f ? 1.0f / l : 0.f;     // ... and the row's probabilities are 0, not 0 / 0
#pragma unroll
            for (int kt = 0; kt < 6; ++kt)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sc[kt][kb][e] *= inv;
            if (l4 == 0) { sM[qrow] = m; sInv[qrow] = inv; }
        }
        // ctx = hm (P o m / (1 - p)) V, so dP = hm m / (1 - p) o (dO V^T); without hm here
        const uint32_t dbase = attn_drop_base((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qrow), (uint32_t)l4, p.drop_key);
        auto dp_masked = [&](int kt, int kb) {
            const int krow = kt * 32 + kb * 16;
            const bf16x8 fv0 = *reinterpret_cast<const bf16x8*>(img1 + swz128(krow + l15, l4));
            const bf16x8 fv1 = *reinterpret_cast<const bf16x8*>(img1 + swz128(krow + l15, 4 + l4));
            f32x4 dp = {0.f, 0.f, 0.f, 0.f};
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv0, fdo[0], dp, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv1, fdo[1], dp, 0, 0, 0);
            if (dthr) {
                const uint32_t hx = attn_drop_word(dbase, (2 * kt + kb) * 2, p.drop_key);
                const uint32_t hy = attn_drop_word(dbase, (2 * kt + kb) * 2 + 1, p.drop_key);
#pragma unroll
                for (int e = 0; e < 4; ++e) dp[e] *= attn_keep_field(hx, hy, e, dthr) ? p.drop_keep : 0.f;
            }
            return dp;
        };
        float dl = 0.f;
#pragma unroll
        for (int kt = 0; kt < 6; ++kt)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const f32x4 dp = dp_masked(kt, kb);
#pragma unroll
                for (int e = 0; e < 4; ++e) dl += sc[kt][kb][e] * dp[e];
                __builtin_amdgcn_sched_barrier(0);
            }
        dl += __shfl_xor(dl, 16, 64);
        dl += __shfl_xor(dl, 32, 64);
        if (l4 == 0) sDl[qrow] = dl;
        f32x4 dq[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) dq[db] = f32x4{0.f, 0.f, 0.f, 0.f};
        // (16-byte stores of d_bias where the row pieces are aligned: L % 4 == 0 and an aligned base)
        const bool dvec = DBIAS && (L & 3) == 0 && ((uintptr_t)p.d_bias & 15) == 0;
#pragma unroll
        for (int kt = 0; kt < 6; ++kt) {
            bf16x8 dsb;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const f32x4 dp = dp_masked(kt, kb);
                f32x4 ds;
#pragma unroll
                for (int e = 0; e < 4; ++e) { ds[e] = sc[kt][kb][e] * (dp[e] - dl); dsb[4 * kb + e] = (bf16)ds[e]; }
                if (DBIAS && qrow < S) {
                    const int key0 = kt * 32 + kb * 16 + 4 * l4;
                    float* at = dbias + (int64_t)qrow * L + key0;
                    if (dvec && key0 < L) *reinterpret_cast<f32x4*>(at) = ds * hm;
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (key0 + e < L) at[e] = ds[e] * hm;
                }
            }
#pragma unroll
            for (int db = 0; db < 4; ++db)
                dq[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abb_tr8(img0, kt * 32, db, l15, l4), dsb, dq[db], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        const float qscale = 0.125f * hm;
        if (qrow < S) {
            bf16* oq = reinterpret_cast<bf16*>(p.dqkv) + ((int64_t)n * S + qrow) * 3 * H + a * 64 + 4 * l4;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const f32x4 o = dq[db];
                *reinterpret_cast<bf16x4*>(oq + db * 16) =
                    bf16x4{(bf16)(o[0] * qscale), (bf16)(o[1] * qscale), (bf16)(o[2] * qscale), (bf16)(o[3] * qscale)};
            }
        }
    }
    __syncthreads();
    if constexpr (DHM) {
        // d_hm = sum_i dctx_i . (P'.V)_i = sum_i sum_j P_ij (m_ij / (1 - p)) (dctx_i . v_j): the sum over the S real query rows of the
        // delta sub-pass Q left in sDl, which carries no hm (hm enters at the stores only), so hm = 0 keeps its gradient.  A row whose
        // every key is -inf left P = 0 and delta = 0; rows beyond S are not read.  One wave, a fixed order (three rows per lane in
        // ascending order, then the butterfly), one store: two launches are bit-identical.
        if (wave == 0) {
            float g = 0.f;
#pragma unroll
            for (int r = 0; r < LP / 64; ++r) {
                const int i = r * 64 + lane;
                if (i < S) g += sDl[i];
            }
            g = wave_sum(g);
            if (lane == 0) p.d_head_mask[n * p.A + a] = g;
        }
    }
    // ---- images of sub-pass K: Qs rows, dO rows (S of them) -------------------------------------------------------
    for (int it = tid; it < LP * 8; it += ABB::NT) {
        const int t = it >> 3, c = it & 7;
        put_rows(img0, t, c, q8(t, c));
        put_rows(img1, t, c, do8(t, c));
    }
    __syncthreads();
    const int qtiles = PREFIX ? (S + 31) >> 5 : 6;          // with prefix rows: the 32-query tiles that hold a query
    // ---- sub-pass K: one 16-key block at a time; with prefix rows the blocks beyond L (no key) are skipped -----------------
#pragma unroll 1
    for (int kb = 0; kb < 2; ++kb) {
        if (PREFIX && t0 + kb * 16 >= L) break;
        const int key = t0 + kb * 16 + l15_;
        bf16x8 fkk[2], fvv[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            fkk[ks] = kv8(key, 0, ks * 4 + l4_);
            fvv[ks] = kv8(key, 1, ks * 4 + l4_);
        }
        f32x4 dk[4], dv[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) { dk[db] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const float kpad = key < L ? 0.f : -INFINITY;
        const int keyc = min(key, L - 1);
#pragma unroll 1
        for (int qt = 0; qt < qtiles; ++qt) {
            int l15 = l15_, l4 = l4_;
            asm volatile("" : "+v"(l15), "+v"(l4));
            // the lane's bias values of the 32-query tile: key `key`, queries 32 qt + 16 qb + 4 l4 + {0..3} (a padded query takes row
            // S - 1, as in sub-pass Q); requested ahead of the products, added after them
            f32x4 bq[2];
            if constexpr (BIAS) {
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) bq[qb][e] = bias[(uint32_t)min(qt * 32 + qb * 16 + 4 * l4 + e, S - 1) * bsq + (uint32_t)keyc];
            }
            bf16x8 pB, dsB;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                const int qrow = qt * 32 + qb * 16;
                const bf16x8 fq0 = *reinterpret_cast<const bf16x8*>(img0 + swz128(qrow + l15, l4));
                const bf16x8 fq1 = *reinterpret_cast<const bf16x8*>(img0 + swz128(qrow + l15, 4 + l4));
                const bf16x8 fd0 = *reinterpret_cast<const bf16x8*>(img1 + swz128(qrow + l15, l4));
                const bf16x8 fd1 = *reinterpret_cast<const bf16x8*>(img1 + swz128(qrow + l15, 4 + l4));
                const f32x4 m4 = *reinterpret_cast<const f32x4*>(sM + qrow + 4 * l4);
                const f32x4 i4 = *reinterpret_cast<const f32x4*>(sInv + qrow + 4 * l4);
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(sDl + qrow + 4 * l4);
                f32x4 c = {kpad, kpad, kpad, kpad};
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq0, fkk[0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq1, fkk[1], c, 0, 0, 0);
                f32x4 dp = {0.f, 0.f, 0.f, 0.f};
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd0, fvv[0], dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd1, fvv[1], dp, 0, 0, 0);
                // dropout: a lane's four values are four queries of ONE key, four hash counters; each lane of a quad hashes one
                // and they are exchanged by quad broadcasts (attn_bwd_mfma_kernel)
                uint32_t hqx = 0, hqy = 0;
                if (dthr) attn_drop_words((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qrow + 4 * l4 + (l15 & 3)), key >> 2, p.drop_key, hqx, hqy);
                const uint32_t xq[4] = {quad_bcast<0>(hqx), quad_bcast<1>(hqx), quad_bcast<2>(hqx), quad_bcast<3>(hqx)};
                const uint32_t yq[4] = {quad_bcast<0>(hqy), quad_bcast<1>(hqy), quad_bcast<2>(hqy), quad_bcast<3>(hqy)};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(BIAS ? fmaf(bq[qb][e], LOG2E, c[e] - m4[e]) : c[e] - m4[e]) * i4[e];
                    float mk = 1.0f;                        // dropout factor of (query qrow + 4 l4 + e, key)
                    if (dthr) mk = attn_keep_field(xq[e], yq[e], key & 3, dthr) ? p.drop_keep : 0.f;
                    pB[4 * qb + e] = (bf16)(pe * mk);       // dV takes the masked probabilities
                    dsB[4 * qb + e] = (bf16)(pe * (mk * dp[e] - d4[e]));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const bf16x8 qf = abb_tr8(img0, qt * 32, db, l15, l4), df = abb_tr8(img1, qt * 32, db, l15, l4);
                dv[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, pB, dv[db], 0, 0, 0);
                dk[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, dsB, dk[db], 0, 0, 0);
            }
        }
        if (key < L) {
            // the key's dk | dv row: a prefix key's in the prefix gradient rows [N*P][2H], an own key's in dq | dk | dv [N*S][3H]
            bf16* ob = key < P ? reinterpret_cast<bf16*>(p.dkvh) + ((int64_t)n * P + key) * 2 * H
                               : reinterpret_cast<bf16*>(p.dqkv) + ((int64_t)n * S + (key - P)) * 3 * H + H;
            ob += a * 64 + 4 * l4_;
            const float kscale = hm * (1.0f / LOG2E);
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const f32x4 ok = dk[db], ov = dv[db];
                *reinterpret_cast<bf16x4*>(ob + db * 16) = bf16x4{(bf16)(ok[0] * kscale), (bf16)(ok[1] * kscale), (bf16)(ok[2] * kscale), (bf16)(ok[3] * kscale)};
                *reinterpret_cast<bf16x4*>(ob + H + db * 16) = bf16x4{(bf16)(ov[0] * hm), (bf16)(ov[1] * hm), (bf16)(ov[2] * hm), (bf16)(ov[3] * hm)};
            }
        }
    }
}

// ---- exact fp32 (VALU): one block (4 waves) per (n, head), L <= 256; attn_bwd_f32_kernel with the bias in the scores -------------
// Pass A (K, V of the L keys in LDS; one query per wave-iteration, S of them): p_ij, dp_ij, delta_i, ds_ij (-> d_bias row i), dQ_i;
// (max, 1 / sum, delta) of every query row stay in LDS.  Pass B (Q, dO of the S queries in LDS; one key per wave-iteration, L of
// them): p and ds rebuilt from them, dV_j and dK_j to the prefix or the own rows.
template <bool PREFIX, typename TD, bool DHM>
__global__ __launch_bounds__(256) void attn_bias_bwd_f32_kernel(AttnBiasBwdArgs p) {
    extern __shared__ float sm[];
    const int S = p.S, P = PREFIX ? p.P : 0, L = S + P, H = p.H;
    float* sA = sm;                          // pass A: K [L][65]   | pass B: Q  [S][65]
    float* sB = sA + (size_t)L * 65;         // pass A: V [L][65]   | pass B: dO [S][65]
    float* sMx = sB + (size_t)L * 65;        // row max, 1 / row sum, delta  [3][S]
    float* sInv = sMx + S;
    float* sDl = sInv + S;
    float* sW = sDl + S;                     // per wave: 64 + 64 + L + L floats
    const int n = blockIdx.x / p.A, a = blockIdx.x % p.A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* wq = sW + (size_t)wave * (128 + 2 * L);      // query row (A) / key row (B)
    float* wd = wq + 64;                                 // dO row (A) / value row (B)
    float* wp = wd + 64;                                 // p_j (B: p_i)
    float* ws = wp + L;                                  // ds_j (B: ds_i)
    const float* qkv = reinterpret_cast<const float*>(p.qkv) + (int64_t)n * S * 3 * H + a * 64;
    const float* kvh = reinterpret_cast<const float*>(p.kvh) + (int64_t)n * P * 2 * H + a * 64;
    const TD* dctx = reinterpret_cast<const TD*>(p.dctx) + (int64_t)n * S * H + a * 64;
    float* dqkv = reinterpret_cast<float*>(p.dqkv) + (int64_t)n * S * 3 * H + a * 64;
    float* dkvh = reinterpret_cast<float*>(p.dkvh) + (int64_t)n * P * 2 * H + a * 64;
    const float* bias = p.bias ? p.bias + (int64_t)n * p.bias_sn + (int64_t)a * p.bias_sa : nullptr;
    float* dbias = p.d_bias ? p.d_bias + ((int64_t)n * p.A + a) * S * L : nullptr;
    auto bias_at = [&](int i, int j) { return bias ? bias[(int64_t)i * p.bias_sq + j] : 0.f; };
    // key j's k row (its v row H further): prefix rows first, then the own rows
    auto krow = [&](int j) { return j < P ? kvh + (int64_t)j * 2 * H : qkv + (int64_t)(j - P) * 3 * H + H; };
    const uint32_t dthr = p.drop_thr16;
    const float keepv = (p.head_mask ? p.head_mask[(int64_t)n * p.head_mask_sn + a] : 1.0f) * (dthr ? p.drop_keep : 1.0f);
    auto dmask = [&](int i, int j) {        // hm x keep / (1 - p) of weight (query i, key j)
        if (!dthr) return keepv;
        uint32_t hx, hy;
        attn_drop_words((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + i), j >> 2, p.drop_key, hx, hy);
        return attn_keep_field(hx, hy, j & 3, dthr) ? keepv : 0.f;
    };
    // DHM: the same weight's factor WITHOUT hm, keep / (1 - p), next to it (one hash for both); keepv stays folded as it is --
    // (hm keep) x and hm (keep x) round differently
    const float keep1 = dthr ? p.drop_keep : 1.0f;
    auto dmask2 = [&](int i, int j, float& m1) {
        m1 = keep1;
        if (!dthr) return keepv;
        uint32_t hx, hy;
        attn_drop_words((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + i), j >> 2, p.drop_key, hx, hy);
        const bool kept = attn_keep_field(hx, hy, j & 3, dthr);
        if (!kept) m1 = 0.f;
        return kept ? keepv : 0.f;
    };
    float ghm = 0.f;                         // DHM: this lane's share of d_hm, over its keys of every query row of the wave
    // ---- pass A ------------------------------------------------------------------------------------------
    for (int idx = tid; idx < L * 64; idx += 256) {
        const int j = idx >> 6, d = idx & 63;
        const float* r = krow(j);
        sA[j * 65 + d] = r[d];
        sB[j * 65 + d] = r[H + d];
    }
    __syncthreads();
    for (int i = wave; i < S; i += 4) {
        wq[lane] = qkv[(int64_t)i * 3 * H + lane];
        wd[lane] = to_f32(dctx[(int64_t)i * H + lane]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float sv[4], dp[4], dp1[4], mx = -INFINITY;         // dp1 (DHM): dp without hm
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = lane + 64 * c;
            sv[c] = -INFINITY; dp[c] = 0.f; dp1[c] = 0.f;
            if (j < L) {
                float s = 0.f, t = 0.f;
                for (int d = 0; d < 64; ++d) { s = fmaf(wq[d], sA[j * 65 + d], s); t = fmaf(wd[d], sB[j * 65 + d], t); }
                s = s / 8.0f + bias_at(i, j);
                sv[c] = s;
                if constexpr (DHM) {
                    float m1;
                    dp[c] = t * dmask2(i, j, m1);
                    dp1[c] = t * m1;
                } else {
                    dp[c] = t * dmask(i, j);
                }
                mx = fmaxf(mx, s);
            }
        }
        mx = wave_max(mx);
        if (mx == -INFINITY) mx = 0.f;      // every key at -inf: the row's probabilities are 0
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (lane + 64 * c < L) { sv[c] = expf(sv[c] - mx); sum += sv[c]; }
        sum = wave_sum(sum);
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;
        float dl = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (lane + 64 * c < L) { sv[c] *= inv; dl += sv[c] * dp[c]; }
        dl = wave_sum(dl);
        if constexpr (DHM) {                // p_ij (kept ? 1 / (1 - p) : 0) (dctx_i . v_j); a row of -inf keys has p = 0
#pragma unroll
            for (int c = 0; c < 4; ++c) if (lane + 64 * c < L) ghm += sv[c] * dp1[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (lane + 64 * c < L) {
                const float ds = sv[c] * (dp[c] - dl);
                ws[lane + 64 * c] = ds;
                if (dbias) dbias[(int64_t)i * L + lane + 64 * c] = ds;
            }
        if (lane == 0) { sMx[i] = mx; sInv[i] = inv; sDl[i] = dl; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float g = 0.f;
        for (int j = 0; j < L; ++j) g = fmaf(ws[j], sA[j * 65 + lane], g);
        dqkv[(int64_t)i * 3 * H + lane] = g / 8.0f;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    if constexpr (DHM) {
        // the waves' sums through the head of their own row buffers (free until pass B fills them, behind the second barrier
        // below), added in wave order by one lane
        ghm = wave_sum(ghm);
        if (lane == 0) wq[0] = ghm;
    }
    __syncthreads();
    if constexpr (DHM) {
        if (tid == 0) {
            float g = 0.f;
            for (int w = 0; w < 4; ++w) g += sW[(size_t)w * (128 + 2 * L)];
            p.d_head_mask[n * p.A + a] = g;
        }
    }
    // ---- pass B ------------------------------------------------------------------------------------------
    for (int idx = tid; idx < S * 64; idx += 256) {
        const int i = idx >> 6, d = idx & 63;
        sA[i * 65 + d] = qkv[(int64_t)i * 3 * H + d];
        sB[i * 65 + d] = to_f32(dctx[(int64_t)i * H + d]);
    }
    __syncthreads();
    for (int j = wave; j < L; j += 4) {
        const float* r = krow(j);
        wq[lane] = r[lane];
        wd[lane] = r[H + lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = lane + 64 * c;
            if (i < S) {
                float s = 0.f, t = 0.f;
                for (int d = 0; d < 64; ++d) { s = fmaf(sA[i * 65 + d], wq[d], s); t = fmaf(sB[i * 65 + d], wd[d], t); }
                s = s / 8.0f + bias_at(i, j);
                const float pij = expf(s - sMx[i]) * sInv[i];
                const float mij = dmask(i, j);
                wp[i] = pij * mij;
                ws[i] = pij * (t * mij - sDl[i]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float gv = 0.f, gk = 0.f;
        for (int i = 0; i < S; ++i) { gv = fmaf(wp[i], sB[i * 65 + lane], gv); gk = fmaf(ws[i], sA[i * 65 + lane], gk); }
        float* o = j < P ? dkvh + (int64_t)j * 2 * H : dqkv + (int64_t)(j - P) * 3 * H + H;
        o[lane] = gk / 8.0f;
        o[H + lane] = gv;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

template <typename K>
int abb_configure(K kernel, int bytes, bool& configured) {
    if (configured) return MODCR_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        modcr_set_error("attn_bias_bwd: cannot reserve %d bytes of LDS: %s", bytes, hipGetErrorString(e));
        return MODCR_ERR_LAUNCH;
    }
    configured = true;
    return MODCR_OK;
}

template <bool PREFIX, bool BIAS, bool DBIAS, bool DHM>
int launch_mfma(const AttnBiasBwdArgs& b, hipStream_t st) {
    static bool configured_dev[MODCR_MAX_DEV] = {};
    const int rc = abb_configure(&attn_bias_bwd_mfma_kernel<PREFIX, BIAS, DBIAS, DHM>, ABB::SMEM, configured_dev[modcr_device_index()]);
    if (rc != MODCR_OK) return rc;
    hipLaunchKernelGGL((attn_bias_bwd_mfma_kernel<PREFIX, BIAS, DBIAS, DHM>), dim3(b.N * b.A), dim3(ABB::NT), ABB::SMEM, st, b);
    return modcr_check_launch("attn_bias_bwd_mfma");
}

template <bool PREFIX, typename TD, bool DHM>
int launch_f32(const AttnBiasBwdArgs& b, hipStream_t st) {
    static bool configured_dev[MODCR_MAX_DEV] = {};
    const int rc = abb_configure(&attn_bias_bwd_f32_kernel<PREFIX, TD, DHM>, 160 * 1024, configured_dev[modcr_device_index()]);
    if (rc != MODCR_OK) return rc;
    const size_t S = (size_t)b.S, L = (size_t)b.S + (size_t)b.P;
    const size_t smem = (2 * L * 65 + 3 * S + 4 * (128 + 2 * L)) * sizeof(float);         // 146 KB at S = L = 256
    hipLaunchKernelGGL((attn_bias_bwd_f32_kernel<PREFIX, TD, DHM>), dim3(b.N * b.A), dim3(256), smem, st, b);
    return modcr_check_launch("attn_bias_bwd_f32");
}

template <bool PREFIX, bool DHM>
int launch(const AttnBiasBwdArgs& b, int core, int32_t dtype, hipStream_t st) {
    if (core != 1) return dtype == MODCR_BF16 ? launch_f32<PREFIX, bf16, DHM>(b, st) : launch_f32<PREFIX, float, DHM>(b, st);
    if (!b.bias) return launch_mfma<PREFIX, false, false, DHM>(b, st);
    return b.d_bias ? launch_mfma<PREFIX, true, true, DHM>(b, st) : launch_mfma<PREFIX, true, false, DHM>(b, st);
}

}  // namespace

int modcr_launch_attn_bias_bwd(const AttnBiasBwdArgs& b, int core, int32_t dtype, hipStream_t stream) {
    const bool prefix = b.P > 0;
    MODCR_REQUIRE(b.qkv && b.dctx && b.dqkv && (b.kvh != nullptr) == prefix && (b.dkvh != nullptr) == prefix && (b.bias || b.head_mask || b.d_head_mask) &&
                      (b.bias || !b.d_bias),
                  "attn_bias_bwd: null pointer");
    MODCR_REQUIRE(b.N > 0 && b.A > 0 && b.H == b.A * 64 && b.S > 0 && b.P >= 0 && (int64_t)b.S + b.P <= (core == 1 ? ABB::LP : 256),
                  "attn_bias_bwd: unsupported call (S=%d P=%d)", b.S, b.P);
    if (core == 1)
        MODCR_REQUIRE(dtype == MODCR_BF16 && modcr_aligned16(b.qkv) && modcr_aligned16(b.kvh) && modcr_aligned16(b.dctx) && modcr_aligned16(b.dqkv) &&
                          modcr_aligned16(b.dkvh),
                      "attn_bias_bwd: the MFMA core takes 16-byte aligned bf16 rows");
    if (b.d_head_mask) return prefix ? launch<true, true>(b, core, dtype, stream) : launch<false, true>(b, core, dtype, stream);
    return prefix ? launch<true, false>(b, core, dtype, stream) : launch<false, false>(b, core, dtype, stream);
}
