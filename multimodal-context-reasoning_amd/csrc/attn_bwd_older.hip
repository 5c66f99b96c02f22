// The older cores of the attention backward under binary masks (CDNA4 / gfx950; no prefix rows, S <= 256), from recomputed q | k | v rows and
// dctx alone -- no saved row statistics, eight products per (query block, key block):
//   attn_bwd_mfma_kernel<bf16, DALIGN>  bf16 rows in and out on the matrix pipe, S <= 192; DALIGN = the align map's gradient rides in
//   attn_bwd_f32_kernel<TD>             the exact fp32 VALU core: S <= 256, the fp32 parity path, and bf16 beyond the MFMA tile
// The five-product core that replaces the first wherever the forward saved lse (and a dump, for d_align) is attn_bwd.hip's.  A file of
// their own rather than a section of attn_bwd.hip: the dropout-mask helpers of attn_common.h have internal linkage, and the compiler
// specialises them to the argument ranges of all their callers in a translation unit -- beside these kernels' calls the instruction stream
// of attn_bwd5_kernel / attn_bwd6_kernel<.., DROP = 1> changes.
#include "common.h"
#include "attn_common.h"

namespace {

// ---- attention core backward on the matrix pipe (bf16 path, S <= 192): one workgroup of 6 waves per (n, head) -------
// Same inputs / outputs as attn_bwd_f32_kernel below (recomputed fp32 q|k|v rows, dctx -> fp32 dq|dk|dv rows).
// Wave w owns tokens 32 w .. 32 w + 31 twice:
//   sub-pass Q (its QUERIES; K rows, V rows and K^T in LDS): S^T = K.Qs^T for all 192 keys stays in registers
//     (Qs = Q log2e / 8, mask = accumulator init) -> exact row max / sum -> P^T; delta = rowsum(P o dP) with
//     dP^T = V.dO^T; then dS^T = P^T o (dP^T - delta), whose bf16 pairs are the B operand of dQ^T += K^T.dS^T
//     (accumulator as operand, keys permuted identically on the K^T fragment reads).  Row statistics go to LDS.
//   sub-pass K (its KEYS; Qs rows, dO rows, Qs^T, dO^T in LDS): per 32-query tile S = Qs.K^T and dP = dO.V^T with
//     the query in the registers, P and dS rebuilt from the row statistics, dV^T += dO^T.P, dK^T += Qs^T.dS.
// Padding: dO rows beyond S are zero (their P, dS contribute nothing), keys beyond S carry a -inf mask.
struct AB {
    static constexpr int LP = ATTN_BWD_MFMA_LP, NT = 384;
    static constexpr int ROWS = LP * 128;                   // [token][64] bf16, 128-byte rows, swz128
    // The transposed operands (K^T; Qs^T, dO^T) are NOT kept as images: ds_read_b64_tr_b16 reads them out of the row images
    // (a lane receives four consecutive tokens of one feature = half an MFMA operand).  Round 1 built [d][token] copies with
    // eight 2-byte LDS stores per 16-byte piece and needed 108 KB per workgroup (one workgroup of six waves per CU);
    // 57 KB now, two workgroups per CU.
    static constexpr int IMG = 2 * ROWS;                    // sub-pass Q: K | V    sub-pass K: Qs | dO
    static constexpr int SMEM = IMG + 4 * LP * 4 + LP * 6 * 4;
};

// DALIGN: the align map's gradient rides in (seq_enc layers 9-11 of the trainable-encoder variant only).  A template parameter:
// as a run-time branch its per-block address arithmetic was hoisted to the top of the kernel and spilled (85 scratch stores
// before the first MFMA) in every call.
template <typename TD, bool DALIGN>
__global__ __launch_bounds__(384, 3) void attn_bwd_mfma_kernel(AttnBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int LP = AB::LP;
    unsigned char* img0 = smem;                             // rows image 0 (K | Qs)
    unsigned char* img1 = smem + AB::ROWS;                  // rows image 1 (V | dO)
    float* sM = reinterpret_cast<float*>(smem + AB::IMG);
    float* sInv = sM + LP;
    float* sDl = sInv + LP;
    float* sMask = sDl + LP;
    uint32_t* sBits = reinterpret_cast<uint32_t*>(sMask + LP);
    const int S = p.S, H = p.H;
    const int n = blockIdx.x / p.A, a = blockIdx.x % p.A;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15_ = lane & 15, l4_ = lane >> 4;
    const int LW = (S + 31) >> 5;
    const bf16* qkv = p.qkvb + (int64_t)n * S * 3 * H + a * 64;
    const TD* dctx = reinterpret_cast<const TD*>(p.dctx) + (int64_t)n * S * H + a * 64;
    float* dqkv = p.dqkv + (int64_t)n * S * 3 * H + a * 64;
    constexpr float QS = 0.125f * LOG2E;

    // 8 consecutive features of token t (zeros beyond S) from the bf16 q|k|v rows (k, v: as they are -- the values the forward's
    // images held; q: scaled by log2e / 8 and rounded again) or from dctx
    auto row8 = [&](int t, int part, int c, float scale) {
        bf16x8 o;
        if (t < S) {
            o = *reinterpret_cast<const bf16x8*>(qkv + (int64_t)t * 3 * H + part * H + c * 8);
            if (scale != 1.0f) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)o[e] * scale);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)0.f;
        }
        return o;
    };
    auto do8 = [&](int t, int c) {
        bf16x8 o;
        if (t < S) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)to_f32(dctx[(int64_t)t * H + c * 8 + e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)0.f;
        }
        return o;
    };
    auto put_rows = [&](unsigned char* img, int t, int c, const bf16x8& v) { *reinterpret_cast<bf16x8*>(img + swz128(t, c)) = v; };
    // Transposed fragment of a row image: feature 16 db + l15, tokens tok0 + 4 l4 + {0..3} and tok0 + 16 + 4 l4 + {0..3} (the key
    // order of the accumulator-as-operand products).  Within a 16-lane group lane i addresses token row (i >> 2), 8-byte piece
    // (i & 3) of the 16-feature span and receives feature i (tools: transpose64_kernel, the TN GEMM); swz128 is applied per lane.
    typedef __attribute__((address_space(3))) bf16x4* lds_tr;
    auto tr8 = [&](const unsigned char* img, int tok0, int db, int l15, int l4) {
        const int r = tok0 + 4 * l4 + (l15 >> 2);
        const int ch = db * 2 + ((l15 & 3) >> 1), within = (l15 & 1) * 8;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr)(img + swz128(r, ch) + within));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr)(img + swz128(r + 16, ch) + within));
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
        return o;
    };

    // ---- tables and the images of sub-pass Q ---------------------------------------------------------------
    for (int j = tid; j < LP; j += AB::NT) {
        float m;
        if (j >= S) m = -INFINITY;
        else if (p.bits) m = 0.f;
        else m = (1.0f - p.key_mask[(int64_t)n * S + j]) * (MODCR_NEG * LOG2E);
        sMask[j] = m;
    }
    if (p.bits)
        for (int j = tid; j < LP * 6; j += AB::NT) {
            const int q = j / 6, w = j % 6;
            sBits[j] = (q < S && w < LW) ? p.bits[((int64_t)n * S + q) * LW + w] : 0xffffffffu;
        }
    for (int it = tid; it < LP * 8; it += AB::NT) {
        const int t = it >> 3, c = it & 7;
        put_rows(img0, t, c, row8(t, 1, c, 1.0f));
        put_rows(img1, t, c, row8(t, 2, c, 1.0f));
    }
    __syncthreads();

    const int t0 = wave * 32;                               // this wave's tokens
    if (MODCR_DBG(p.debug & 1)) return;
    // ---- sub-pass Q ------------------------------------------------------------------------------------------
    // One 16-query block at a time (its 16 x 192 scores = 48 registers): with both blocks of the wave's 32 queries unrolled
    // side by side the kernel took 256 registers + 42 spilled, one workgroup per CU; the K / V / K^T fragments are read twice.
    if (!MODCR_DBG(p.debug & 2)) {
#pragma unroll 1
        for (int qb = 0; qb < 2; ++qb) {
            // per-iteration opaque copies of the lane indices: the fragment addresses below are loop invariant, and hoisted out
            // of this loop their ~100 registers were spilled ahead of the first MFMA
            int l15 = l15_, l4 = l4_;
            asm volatile("" : "+v"(l15), "+v"(l4));
            const int qrow = t0 + qb * 16 + l15;
            bf16x8 fq[2], fdo[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                fq[ks] = row8(qrow, 0, ks * 4 + l4, QS);            // zeros beyond S, as the Qs image of sub-pass K (same row statistics)
                fdo[ks] = do8(qrow, ks * 4 + l4);
            }
            f32x4 sc[6][2];
#pragma unroll
            for (int kt = 0; kt < 6; ++kt)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const int krow = kt * 32 + kb * 16;
                    const bf16x8 fk0 = *reinterpret_cast<const bf16x8*>(img0 + swz128(krow + l15, l4));
                    const bf16x8 fk1 = *reinterpret_cast<const bf16x8*>(img0 + swz128(krow + l15, 4 + l4));
                    f32x4 c = *reinterpret_cast<const f32x4*>(sMask + krow + 4 * l4);
                    if (p.bits) {
                        const uint32_t word = sBits[qrow * 6 + kt];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (!((word >> (kb * 16 + 4 * l4 + e)) & 1u)) c[e] += MODCR_NEG * LOG2E;
                    }
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk0, fq[0], c, 0, 0, 0);
                    sc[kt][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk1, fq[1], c, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);      // no hoisting of the next blocks' fragment reads: registers
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
                float l = 0.f;
#pragma unroll
                for (int kt = 0; kt < 6; ++kt)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float ex = __builtin_amdgcn_exp2f(sc[kt][kb][e] - m); sc[kt][kb][e] = ex; l += ex; }
                l += __shfl_xor(l, 16, 64);
                l += __shfl_xor(l, 32, 64);
                const float inv = 1.0f / l;
#pragma unroll
                for (int kt = 0; kt < 6; ++kt)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int e = 0; e < 4; ++e) sc[kt][kb][e] *= inv;
                if (l4 == 0) { sM[qrow] = m; sInv[qrow] = inv; }
            }
            // forward dropout on the probabilities: O = (P o m) V with m = keep / (1 - p), so dP = m o (dO V^T) below
            const uint32_t dthr = p.drop_thr16;
            const uint32_t dbase = attn_drop_base((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qrow), (uint32_t)l4, p.drop_key);
            auto dp_masked = [&](int kt, int kb) {
                const int krow = kt * 32 + kb * 16;
                const bf16x8 fv0 = *reinterpret_cast<const bf16x8*>(img1 + swz128(krow + l15, l4));
                const bf16x8 fv1 = *reinterpret_cast<const bf16x8*>(img1 + swz128(krow + l15, 4 + l4));
                f32x4 dp = {0.f, 0.f, 0.f, 0.f};
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv0, fdo[0], dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv1, fdo[1], dp, 0, 0, 0);
                float mk4[4] = {1.f, 1.f, 1.f, 1.f};
                if (dthr) {
                    uint32_t hx, hy;
                    hx = attn_drop_word(dbase, (2 * kt + kb) * 2, p.drop_key);
                    hy = attn_drop_word(dbase, (2 * kt + kb) * 2 + 1, p.drop_key);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { mk4[e] = attn_keep_field(hx, hy, e, dthr) ? p.drop_keep : 0.f; dp[e] *= mk4[e]; }
                }
                if constexpr (DALIGN) {         // the align map's gradient, text query x region key: on the un-dropped probabilities,
                                                // or (side_post_drop: the map summed P o m / (1 - p)) under the same mask
                    const int T = p.align_t, key0 = kt * 32 + kb * 16 + 4 * l4;
                    if (qrow < T && key0 + 3 >= T) {
                        const float* da = p.d_align + ((int64_t)n * T + qrow) * (S - T) - T;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (key0 + e >= T && key0 + e < S) dp[e] += p.side_post_drop ? mk4[e] * da[key0 + e] : da[key0 + e];
                    }
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
#pragma unroll
            for (int kt = 0; kt < 6; ++kt) {
                bf16x8 dsb;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const f32x4 dp = dp_masked(kt, kb);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dsb[4 * kb + e] = (bf16)(sc[kt][kb][e] * (dp[e] - dl));
                }
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    dq[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr8(img0, kt * 32, db, l15, l4), dsb, dq[db], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (qrow < S)
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    f32x4 o = dq[db];
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] *= 0.125f;
                    const int64_t at = (int64_t)qrow * 3 * H + db * 16 + 4 * l4;
                    if (p.out_bf16) *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(p.dqkv) + (int64_t)n * S * 3 * H + a * 64 + at) = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
                    else *reinterpret_cast<f32x4*>(dqkv + at) = o;
                }
        }
    }
    __syncthreads();
    // ---- images of sub-pass K: Qs rows, dO rows, Qs^T, dO^T ------------------------------------------------------
    for (int it = tid; it < LP * 8; it += AB::NT) {
        const int t = it >> 3, c = it & 7;
        put_rows(img0, t, c, row8(t, 0, c, QS));
        put_rows(img1, t, c, do8(t, c));
    }
    __syncthreads();
    // ---- sub-pass K ------------------------------------------------------------------------------------------
    // (one 16-key block at a time, as sub-pass Q: the Qs / dO fragments are read twice)
    if (!MODCR_DBG(p.debug & 4)) {
#pragma unroll 1
        for (int kb = 0; kb < 2; ++kb) {
            const int key = t0 + kb * 16 + l15_;
            bf16x8 fkk[2], fvv[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                fkk[ks] = row8(key, 1, ks * 4 + l4_, 1.0f);
                fvv[ks] = row8(key, 2, ks * 4 + l4_, 1.0f);
            }
            const float mkey = sMask[key];
            f32x4 dk[4], dv[4];
#pragma unroll
            for (int db = 0; db < 4; ++db) { dk[db] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
            for (int qt = 0; qt < 6; ++qt) {
                int l15 = l15_, l4 = l4_;
                asm volatile("" : "+v"(l15), "+v"(l4));
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
                    f32x4 c = {mkey, mkey, mkey, mkey};
                    if (p.bits) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const uint32_t word = sBits[(qrow + 4 * l4 + e) * 6 + (key >> 5)];
                            if (!((word >> (key & 31)) & 1u)) c[e] += MODCR_NEG * LOG2E;
                        }
                    }
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq0, fkk[0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq1, fkk[1], c, 0, 0, 0);
                    f32x4 dp = {0.f, 0.f, 0.f, 0.f};
                    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd0, fvv[0], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd1, fvv[1], dp, 0, 0, 0);
                    // dropout: a lane's four values are four queries of ONE key, i.e. four different hash counters; the
                    // four lanes of a quad (keys of one key group) need the same four, so each hashes one and they are
                    // exchanged by quad broadcasts: one hash per lane instead of four
                    uint32_t hqx = 0, hqy = 0;
                    if (p.drop_thr16)
                        attn_drop_words((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qrow + 4 * l4 + (l15 & 3)), key >> 2, p.drop_key, hqx, hqy);
                    const uint32_t xq[4] = {quad_bcast<0>(hqx), quad_bcast<1>(hqx), quad_bcast<2>(hqx), quad_bcast<3>(hqx)};
                    const uint32_t yq[4] = {quad_bcast<0>(hqy), quad_bcast<1>(hqy), quad_bcast<2>(hqy), quad_bcast<3>(hqy)};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float pe = __builtin_amdgcn_exp2f(c[e] - m4[e]) * i4[e];
                        float mk = 1.0f;                    // dropout factor of (query qrow + 4 l4 + e, key)
                        if (p.drop_thr16)                   // the words of query e were hashed by quad lane e
                            mk = attn_keep_field(xq[e], yq[e], key & 3, p.drop_thr16) ? p.drop_keep : 0.f;
                        float dpe = mk * dp[e];
                        if constexpr (DALIGN) {
                            const int T = p.align_t, qi = qrow + 4 * l4 + e;
                            if (qi < T && key >= T && key < S) {
                                const float da = p.d_align[((int64_t)n * T + qi) * (S - T) + (key - T)];
                                dpe += p.side_post_drop ? mk * da : da;
                            }
                        }
                        pB[4 * qb + e] = (bf16)(pe * mk);                   // dV takes the masked probabilities
                        dsB[4 * qb + e] = (bf16)(pe * (dpe - d4[e]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    const bf16x8 qf = tr8(img0, qt * 32, db, l15, l4), df = tr8(img1, qt * 32, db, l15, l4);
                    dv[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, pB, dv[db], 0, 0, 0);
                    dk[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, dsB, dk[db], 0, 0, 0);
                }
            }
            if (key < S)
#pragma unroll
                for (int db = 0; db < 4; ++db) {
                    f32x4 ok = dk[db];
#pragma unroll
                    for (int e = 0; e < 4; ++e) ok[e] *= (1.0f / LOG2E);
                    const int64_t at = (int64_t)key * 3 * H + H + db * 16 + 4 * l4_;
                    if (p.out_bf16) {
                        bf16* ob = reinterpret_cast<bf16*>(p.dqkv) + (int64_t)n * S * 3 * H + a * 64 + at;
                        const f32x4 ov = dv[db];
                        *reinterpret_cast<bf16x4*>(ob) = bf16x4{(bf16)ok[0], (bf16)ok[1], (bf16)ok[2], (bf16)ok[3]};
                        *reinterpret_cast<bf16x4*>(ob + H) = bf16x4{(bf16)ov[0], (bf16)ov[1], (bf16)ov[2], (bf16)ov[3]};
                    } else {
                        *reinterpret_cast<f32x4*>(dqkv + at) = ok;
                        *reinterpret_cast<f32x4*>(dqkv + at + H) = dv[db];
                    }
                }
        }
    }
}

// ---- attention core backward, exact fp32 (VALU): one block (4 waves) per (n, head) ------------------------------
// From the recomputed q|k|v rows [N,S,3H] (fp32) and dctx: dq|dk|dv rows [N,S,3H] (fp32).  No saved
// probabilities: pass A (K, V in LDS; one query per wave-iteration) recomputes p_ij, forms dp_ij = dO_i.V_j,
// delta_i = sum_j p dp, ds_ij = p (dp - delta) and dQ_i = sum_j ds_ij K_j / 8, keeping (max, 1/sum, delta) of
// every row in LDS; pass B (Q, dO in LDS; one key per wave-iteration) rebuilds p and ds from those row
// statistics and accumulates dV_j = sum_i p_ij dO_i, dK_j = sum_i ds_ij Q_i / 8.  Mask semantics as the forward.

template <typename TD>
__global__ __launch_bounds__(256) void attn_bwd_f32_kernel(AttnBwdArgs p) {
    extern __shared__ float sm[];
    const int S = p.S, H = p.H;
    float* sA = sm;                          // pass A: K   | pass B: Q      [S][65]
    float* sB = sA + (size_t)S * 65;         // pass A: V   | pass B: dO     [S][65]
    float* sMx = sB + (size_t)S * 65;        // row max, 1 / row sum, delta  [3][S]
    float* sInv = sMx + S;
    float* sDl = sInv + S;
    float* sW = sDl + S;                     // per wave: 64 + 64 + S + S floats
    const int n = blockIdx.x / p.A, a = blockIdx.x % p.A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* wq = sW + (size_t)wave * (128 + 2 * S);      // query row (A) / key row (B)
    float* wd = wq + 64;                                 // dO row (A) / value row (B)
    float* wp = wd + 64;                                 // p_j (B: p_i)
    float* ws = wp + S;                                  // ds_j (B: ds_i)
    const int LW = (S + 31) >> 5;
    const float* qkv = p.qkv + (int64_t)n * S * 3 * H;
    const TD* dctx = reinterpret_cast<const TD*>(p.dctx) + (int64_t)n * S * H;
    float* dqkv = p.dqkv + (int64_t)n * S * 3 * H;
    auto seen = [&](int i, int j) {
        if (p.bits) return ((p.bits[((int64_t)n * S + i) * LW + (j >> 5)] >> (j & 31)) & 1u) != 0;
        return p.key_mask[(int64_t)n * S + j] != 0.f;
    };
    auto dalign = [&](int i, int j) {       // gradient arriving through the align map
        const int T = p.align_t;
        return (p.d_align && i < T && j >= T) ? p.d_align[((int64_t)n * T + i) * (S - T) + (j - T)] : 0.f;
    };
    // the forward's attention-probability dropout (tile kernels, csrc/attn_common.h): keep / (1 - p) of weight (i, j), regenerated
    // from its counter layout -- ctx = (P o m) V, so dP = m o (dO V^T) and dV = (P o m)^T dO; the align map saw the unmasked P
    const uint32_t dthr = p.drop_thr16;
    auto dmask = [&](int i, int j) {
        if (!dthr) return 1.0f;
        uint32_t hx, hy;
        attn_drop_words((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + i), j >> 2, p.drop_key, hx, hy);
        return attn_keep_field(hx, hy, j & 3, dthr) ? p.drop_keep : 0.f;
    };
    // ---- pass A ------------------------------------------------------------------------------------------
    for (int idx = tid; idx < S * 64; idx += 256) {
        const int j = idx >> 6, d = idx & 63;
        sA[j * 65 + d] = qkv[(int64_t)j * 3 * H + H + a * 64 + d];
        sB[j * 65 + d] = qkv[(int64_t)j * 3 * H + 2 * H + a * 64 + d];
    }
    __syncthreads();
    for (int i = wave; i < S; i += 4) {
        wq[lane] = qkv[(int64_t)i * 3 * H + a * 64 + lane];
        wd[lane] = to_f32(dctx[(int64_t)i * H + a * 64 + lane]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float sv[4], dp[4], mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = lane + 64 * c;
            sv[c] = -INFINITY; dp[c] = 0.f;
            if (j < S) {
                float s = 0.f, t = 0.f;
                for (int d = 0; d < 64; ++d) { s = fmaf(wq[d], sA[j * 65 + d], s); t = fmaf(wd[d], sB[j * 65 + d], t); }
                s = s / 8.0f + (seen(i, j) ? 0.f : MODCR_NEG);
                sv[c] = s; dp[c] = p.side_post_drop ? (t + dalign(i, j)) * dmask(i, j) : t * dmask(i, j) + dalign(i, j);
                mx = fmaxf(mx, s);
            }
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (lane + 64 * c < S) { sv[c] = expf(sv[c] - mx); sum += sv[c]; }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
        float dl = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (lane + 64 * c < S) { sv[c] *= inv; dl += sv[c] * dp[c]; }
        dl = wave_sum(dl);
#pragma unroll
        for (int c = 0; c < 4; ++c) if (lane + 64 * c < S) ws[lane + 64 * c] = sv[c] * (dp[c] - dl);
        if (lane == 0) { sMx[i] = mx; sInv[i] = inv; sDl[i] = dl; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float g = 0.f;
        for (int j = 0; j < S; ++j) g = fmaf(ws[j], sA[j * 65 + lane], g);
        dqkv[(int64_t)i * 3 * H + a * 64 + lane] = g / 8.0f;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    __syncthreads();
    // ---- pass B ------------------------------------------------------------------------------------------
    for (int idx = tid; idx < S * 64; idx += 256) {
        const int i = idx >> 6, d = idx & 63;
        sA[i * 65 + d] = qkv[(int64_t)i * 3 * H + a * 64 + d];
        sB[i * 65 + d] = to_f32(dctx[(int64_t)i * H + a * 64 + d]);
    }
    __syncthreads();
    for (int j = wave; j < S; j += 4) {
        wq[lane] = qkv[(int64_t)j * 3 * H + H + a * 64 + lane];
        wd[lane] = qkv[(int64_t)j * 3 * H + 2 * H + a * 64 + lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = lane + 64 * c;
            if (i < S) {
                float s = 0.f, t = 0.f;
                for (int d = 0; d < 64; ++d) { s = fmaf(sA[i * 65 + d], wq[d], s); t = fmaf(sB[i * 65 + d], wd[d], t); }
                s = s / 8.0f + (seen(i, j) ? 0.f : MODCR_NEG);
                const float pij = expf(s - sMx[i]) * sInv[i];
                const float mij = dmask(i, j);
                wp[i] = pij * mij;
                ws[i] = pij * ((p.side_post_drop ? (t + dalign(i, j)) * mij : t * mij + dalign(i, j)) - sDl[i]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float gv = 0.f, gk = 0.f;
        for (int i = 0; i < S; ++i) { gv = fmaf(wp[i], sB[i * 65 + lane], gv); gk = fmaf(ws[i], sA[i * 65 + lane], gk); }
        dqkv[(int64_t)j * 3 * H + H + a * 64 + lane] = gk / 8.0f;
        dqkv[(int64_t)j * 3 * H + 2 * H + a * 64 + lane] = gv;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

}  // namespace

int modcr_launch_attn_bwd_older(const AttnBwdArgs& b, AttnBwdCore core, int32_t dtype, hipStream_t stream) {
    static bool configured_dev[MODCR_MAX_DEV] = {};
    bool& configured = configured_dev[modcr_device_index()];
    if (!configured) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_f32_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_f32_kernel<bf16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_mfma_kernel<bf16, false>), hipFuncAttributeMaxDynamicSharedMemorySize, AB::SMEM);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_mfma_kernel<bf16, true>), hipFuncAttributeMaxDynamicSharedMemorySize, AB::SMEM);
        configured = true;
    }
    const int N = b.N, S = b.S, A = b.A;
    // exact core: K | V (Q | dO) rows [S][65], three row statistics, a (query, dO, two S-long rows) scratch per wave
    const size_t smem = ((size_t)2 * S * 65 + 3 * (size_t)S + 4 * (128 + 2 * (size_t)S)) * sizeof(float);
    if (core == ATTN_BWD_MFMA_DALIGN) hipLaunchKernelGGL((attn_bwd_mfma_kernel<bf16, true>), dim3(N * A), dim3(AB::NT), AB::SMEM, stream, b);
    else if (core == ATTN_BWD_MFMA) hipLaunchKernelGGL((attn_bwd_mfma_kernel<bf16, false>), dim3(N * A), dim3(AB::NT), AB::SMEM, stream, b);
    else if (dtype == MODCR_BF16) hipLaunchKernelGGL(attn_bwd_f32_kernel<bf16>, dim3(N * A), dim3(256), smem, stream, b);
    else hipLaunchKernelGGL(attn_bwd_f32_kernel<float>, dim3(N * A), dim3(256), smem, stream, b);
    return modcr_check_launch("attn_bwd");
}
