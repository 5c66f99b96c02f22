// Streaming attention core, forward only.  Two uses:
//   * 256 < P + S <= 512 keys with a binary mask (key mask / dense mask bits), no attention-probability dropout (inference /
//     eval mode): modcr_qkv_attn_opt_fwd above the tile kernels' 256 keys;
//   * any P + S <= 512 with an ADDITIVE fp32 bias per (sequence, head, query, key) and / or a per-head multiplier
//     (modcr_qkv_attn_bias_fwd; with attention-probability dropout above 256 keys modcr_qkv_attn_long_drop_fwd): the BIAS
//     instantiations below, see "Bias variant" further down.
//
// The tile kernels of attn.hip hold the whole key row of a head in LDS; above 256 keys it does not fit, so this core
// streams the keys in tiles of 64 with an online softmax (flash-style).  Its inputs are the q | k | v rows the dispatcher
// (modcr_qkv_attn_opt_fwd) projected into the workspace: qx [N*S][3H] (the x rows, chunk-mean queries already applied)
// and qh [N*P][3H] (the prefix rows).  Keys / values of sequence n are [prefix ; x], queries the x rows.
//
// bf16 core: one workgroup of 2 waves per (64-query block, head, sequence); wave w owns queries 32 w .. 32 w + 31 as two
// 16-query blocks whose Q fragments stay in registers.  Per 64-key tile (double-buffered in LDS, the next one in flight in
// registers under the current one's arithmetic):
//   S^T = K.Q^T  with v_mfma_f32_16x16x32_bf16 (A = K rows from LDS, B = the Q fragment): the QUERY lies on the lane
//                (l & 15), a lane holds keys 16 kb + 4 g + i (g = lane >> 4), so a row's max / sum needs two xor shuffles;
//   scores       acc x log2e / 8 + (masked ? -10000 log2e : 0), -inf beyond P + S; running row max and sum in fp32;
//   O^T += V^T.P^T  with P as bf16 straight from the accumulators: the 32 keys of a step arrive in the order 4 g + e |
//                16 + 4 g + e, and the V^T fragment (two ds_read_b64 of a [feature][key] image) uses that order.
// Side outputs (probabilities, align map) come from a second sweep over the K tiles with the final row max and sum, so
// they are exact and a call without them pays nothing.
//
// fp32 parity core: the same tiling with VALU products, 4 waves x 16 queries, key on the lane for the scores and
// feature on the lane for the context.
//
// Bias variant (MODE 1, MODE 2 = with attention-probability dropout): the score of (n, head a, query q, key j) is
//   q.k / 8 x log2e + bias[n sn + a sa + q sq + j] x log2e      (strides in elements, 0 = broadcast, key stride 1)
// A lane's keys of one 16-key block are four consecutive floats: one 16-byte load when the address is 16-byte aligned and the four
// keys are inside the row, four scalar loads otherwise (L % 4 != 0 with sq = L breaks the alignment on odd rows).  The bias of tile
// t + 1 is requested together with its K / V rows and waits in registers under tile t's arithmetic; with sq = 0 it is loaded once per
// tile for both query sub-blocks.  -inf entries are legal: while a row's running max is -inf the exponentials are taken against 0
// (the tile contributes 0, the rescale of the empty accumulators is harmless), and a row whose every key is -inf leaves with context
// 0 and probabilities 0 -- the one deliberate difference from the reference, whose softmax gives NaN there.  A row of -10000
// everywhere is the uniform softmax, as on the binary routes.  head_mask[n hsn + a] (NULL = 1) multiplies the head's probabilities
// after softmax and dropout: the 64 context columns in the epilogue and the side outputs in the second sweep.
// Dropout (MODE 2): the keep decisions of attn_common.h for row counter attn_drop_row(n, A, head, query, P + S) -- stride 256 up to
// 256 keys, the wide layout (stride 512, words up to 63) above, which only modcr_qkv_attn_long_drop_fwd lets through -- keys over
// [prefix ; x]; the lane's g is the layout's l4, so attn_drop8_rt clears the dropped bf16 pairs of the P^T fragments as in the tile
// kernels.  The context is P o m / (1 - p); the side outputs are the un-dropped probabilities, or with side_post_drop the
// post-dropout ones (the second sweep regenerates the keep bits).
// Mask bits on the bias variant (template parameter BITS, modcr_qkv_attn_long_align_fwd; the instantiations without it compile as
// before): bit j of bits[n, q, :] (u32 [N, S, ceil(S / 32)], no prefix rows) adds 0 or -10000 to the bias of (q, j) BEFORE the
// multiplication by log2e, so a call with bits is bit for bit the call with the bits folded into a 0 / -10000 bias.  The two 32-key
// words of a tile and query are loaded as MODE 0 loads them; a padded query row takes row S - 1's words.
#include <hip/hip_ext.h>

#include "common.h"
#include "attn_common.h"

namespace {

constexpr int LG_KS = 72;                       // K image row stride (bf16): 144-byte rows, conflict-free ds_read_b128
constexpr int LG_VS = 68;                       // V^T image row stride (bf16): 136-byte rows, conflict-free ds_read_b64
constexpr int LG_KIMG = 64 * LG_KS;
constexpr int LG_BUF = LG_KIMG + 64 * LG_VS;    // bf16 elements of one K | V^T buffer (17 920 bytes)

template <typename T> __device__ __forceinline__ const T* lg_row(const AttnLongArgs& p, int n, int j) {
    const int64_t h3 = 3 * (int64_t)p.H;
    return j < p.P ? (const T*)p.qh + ((int64_t)n * p.P + j) * h3 : (const T*)p.qx + ((int64_t)n * p.S + (j - p.P)) * h3;
}

// additive mask of key j (< P + S) for query q (< S), log2 domain
__device__ __forceinline__ float lg_mask(const AttnLongArgs& p, int n, int q, int j, int L) {
    bool see;
    if (p.bits) see = (p.bits[((int64_t)n * p.S + q) * ((L + 31) >> 5) + (j >> 5)] >> (j & 31)) & 1u;
    else see = p.key_mask[(int64_t)n * L + j] != 0.f;
    return see ? 0.f : MODCR_NEG * LOG2E;
}

__device__ __forceinline__ uint32_t lg_half(const uint4& v, int e) {
    const uint32_t w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
    return (e & 1) ? (w >> 16) : (w & 0xffffu);
}

// MODE 0 = binary masks (key_mask / bits), 1 = bias / head mask, 2 = the same with dropout.  LDS admits four workgroups per CU = two
// waves per SIMD; the bias instantiations are asked to stay inside that register budget (left alone they take 208-230 VGPRs beside 32
// AGPRs and the ones with side outputs drop to one wave per SIMD; asked, 224-236 unified, no spill).  MODE 0 compiles as before.
template <bool SIDE, int MODE, bool BITS = false>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(MODE != 0 ? 2 : 1))) void attn_long_bf16_kernel(AttnLongArgs p) {
    static_assert(!BITS || MODE != 0, "MODE 0 reads its bits itself");
    __shared__ __attribute__((aligned(16))) bf16 sm[2 * LG_BUF];
    const int S = p.S, L = p.P + S, H = p.H;
    const int n = blockIdx.z, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int ntiles = (L + 63) >> 6;
    const float sc = 0.125f * LOG2E;

    // Q fragments (B operand of S^T): query q0 + 16 qs + l15, features 32 ds + 8 g .. + 7; rows past S read row S - 1
    int qrow[2];
    bf16x8 qf[2][2];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
        qrow[qs] = blockIdx.x * 64 + wave * 32 + qs * 16 + l15;
        const bf16* r = (const bf16*)p.qx + ((int64_t)n * S + (qrow[qs] < S ? qrow[qs] : S - 1)) * 3 * H + a * 64;
#pragma unroll
        for (int ds = 0; ds < 2; ++ds) qf[qs][ds] = *reinterpret_cast<const bf16x8*>(r + 32 * ds + 8 * g);
    }

    // staging: K piece r of thread t = row (t + 128 r) >> 3, 16-byte chunk t & 7; V: keys 4 (t >> 3) .. + 3, chunk t & 7
    uint4 kreg[4], vreg[4];
    auto load = [&](int t, bool with_v) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = t * 64 + ((tid + 128 * r) >> 3);
            kreg[r] = j < L ? *reinterpret_cast<const uint4*>(lg_row<bf16>(p, n, j) + H + a * 64 + (tid & 7) * 8) : make_uint4(0, 0, 0, 0);
        }
        if (with_v) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * 64 + (tid >> 3) * 4 + r;
                vreg[r] = j < L ? *reinterpret_cast<const uint4*>(lg_row<bf16>(p, n, j) + 2 * H + a * 64 + (tid & 7) * 8)
                                : make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store = [&](int b, bool with_v) {
        bf16* K = sm + b * LG_BUF;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<uint4*>(K + ((tid + 128 * r) >> 3) * LG_KS + (tid & 7) * 8) = kreg[r];
        if (with_v) {
            bf16* Vt = K + LG_KIMG;
#pragma unroll
            for (int e = 0; e < 8; ++e) {           // feature 8 (t & 7) + e, keys 4 (t >> 3) .. + 3: one 8-byte piece
                uint2 w;
                w.x = lg_half(vreg[0], e) | (lg_half(vreg[1], e) << 16);
                w.y = lg_half(vreg[2], e) | (lg_half(vreg[3], e) << 16);
                *reinterpret_cast<uint2*>(Vt + ((tid & 7) * 8 + e) * LG_VS + (tid >> 3) * 4) = w;
            }
        }
    };
    // bias variant: the lane's 4 x 4 bias values of a tile per query sub-block (natural-log domain, as given)
    [[maybe_unused]] const float* brow[2] = {nullptr, nullptr};
    [[maybe_unused]] bool bvec[2] = {false, false};
    if constexpr (MODE != 0) {
        if (p.bias) {
#pragma unroll
            for (int qs = 0; qs < 2; ++qs) {
                brow[qs] = p.bias + n * p.bias_sn + a * p.bias_sa + (qrow[qs] < S ? qrow[qs] : S - 1) * p.bias_sq;
                bvec[qs] = (reinterpret_cast<uintptr_t>(brow[qs]) & 15) == 0;
            }
        }
    }
    [[maybe_unused]] auto load_bias = [&](int t, f32x4 (&bb)[2][4]) {
        const int nq = p.bias_sq == 0 ? 1 : 2;      // one bias row for every query: loaded once per tile
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const int j = t * 64 + kb * 16 + 4 * g;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (qs < nq && brow[qs]) {
                    if (bvec[qs] && j + 3 < L) v = *reinterpret_cast<const f32x4*>(brow[qs] + j);
                    else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (j + i < L) v[i] = brow[qs][j + i];
                    }
                }
                bb[qs][kb] = qs < nq ? v : bb[0][kb];
            }
        }
    };
    // S^T of tile t (buffer b) as log2-domain scores: s[qs][kb][i] = key t 64 + 16 kb + 4 g + i, query qrow[qs]
    auto scores = [&](int t, int b, f32x4 (&s)[2][4], [[maybe_unused]] const f32x4 (&bb)[2][4]) {
        const bf16* K = sm + b * LG_BUF;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(K + (kb * 16 + l15) * LG_KS + 8 * g);
            const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(K + (kb * 16 + l15) * LG_KS + 32 + 8 * g);
#pragma unroll
            for (int qs = 0; qs < 2; ++qs) {
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[qs][0], c, 0, 0, 0);
                s[qs][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[qs][1], c, 0, 0, 0);
            }
        }
        if constexpr (MODE != 0) {
            [[maybe_unused]] uint32_t wb[2][2];         // BITS: the two 32-key words of the tile per query (no prefix rows: L = S)
            if constexpr (BITS) {
                const int LW = (L + 31) >> 5;
#pragma unroll
                for (int qs = 0; qs < 2; ++qs) {
                    const uint32_t* row = p.bits + ((int64_t)n * S + (qrow[qs] < S ? qrow[qs] : S - 1)) * LW;
                    wb[qs][0] = row[2 * t];
                    wb[qs][1] = 2 * t + 1 < LW ? row[2 * t + 1] : 0u;
                }
            }
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = t * 64 + kb * 16 + 4 * g + i;
                    const bool in = j < L;
#pragma unroll
                    for (int qs = 0; qs < 2; ++qs) {
                        float bv = bb[qs][kb][i];
                        if constexpr (BITS) bv += ((wb[qs][kb >> 1] >> (j & 31)) & 1u) ? 0.f : MODCR_NEG;
                        s[qs][kb][i] = in ? fmaf(s[qs][kb][i], sc, bv * LOG2E) : -INFINITY;
                    }
                }
            return;
        }
        // dense mask: the two 32-key words of the tile per query; key mask: one value per key
        uint32_t w[2][2] = {{~0u, ~0u}, {~0u, ~0u}};
        if (p.bits) {
            const int LW = (L + 31) >> 5;
#pragma unroll
            for (int qs = 0; qs < 2; ++qs) {
                const uint32_t* row = p.bits + ((int64_t)n * S + (qrow[qs] < S ? qrow[qs] : S - 1)) * LW;
                w[qs][0] = row[2 * t];
                w[qs][1] = 2 * t + 1 < LW ? row[2 * t + 1] : 0u;
            }
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = t * 64 + kb * 16 + 4 * g + i;
                const bool in = j < L;
                const bool km = p.bits || !in || p.key_mask[(int64_t)n * L + j] != 0.f;
#pragma unroll
                for (int qs = 0; qs < 2; ++qs) {
                    const bool see = km && ((w[qs][kb >> 1] >> (j & 31)) & 1u);
                    s[qs][kb][i] = in ? s[qs][kb][i] * sc + (see ? 0.f : MODCR_NEG * LOG2E) : -INFINITY;
                }
            }
    };

    float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.f, 0.f};
    f32x4 o[2][4];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs)
#pragma unroll
        for (int db = 0; db < 4; ++db) o[qs][db] = f32x4{0.f, 0.f, 0.f, 0.f};

    // dropout (MODE 2): the lane's hash base per query sub-block (its g is the layout's l4), the packed threshold
    [[maybe_unused]] uint32_t dbase[2] = {0u, 0u};
    [[maybe_unused]] uint32_t dthr2 = 0u;
    if constexpr (MODE == 2) {
        dthr2 = attn_thrm1_2(p.drop_thr16);
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) dbase[qs] = attn_drop_base(attn_drop_row(n, p.A, a, qrow[qs], L), (uint32_t)g, p.drop_key);
    }

    f32x4 bcur[2][4], bnext[2][4];
    load(0, true);
    if constexpr (MODE != 0) load_bias(0, bnext);
    store(0, true);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int b = t & 1;
        if constexpr (MODE != 0) {
#pragma unroll
            for (int qs = 0; qs < 2; ++qs)
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) bcur[qs][kb] = bnext[qs][kb];
        }
        if (t + 1 < ntiles) {
            load(t + 1, true);
            if constexpr (MODE != 0) load_bias(t + 1, bnext);
        }
        f32x4 s[2][4];
        scores(t, b, s, bcur);
        bf16x8 pb[2][2];                            // P^T fragments: step ks = keys 32 ks + (4 g + e | 16 + 4 g + e)
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[qs][kb][i]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m[qs], mx);
            // bias variant: every key so far at -inf -> exponentials against 0, the tile contributes 0 (no exp2(-inf + inf))
            const float ms = (MODE != 0 && mn == -INFINITY) ? 0.f : mn;
            const float alpha = __builtin_amdgcn_exp2f(m[qs] - ms);
            m[qs] = mn;
            float sum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e = __builtin_amdgcn_exp2f(s[qs][kb][i] - ms);
                    sum += e;
                    pb[qs][kb >> 1][(kb & 1) * 4 + i] = (bf16)e;
                }
            if constexpr (MODE == 2) {                  // the row sum keeps the un-dropped weights; the context takes P o m
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) pb[qs][ks] = attn_drop8_rt(pb[qs][ks], dbase[qs], 2 * t + ks, p.drop_key, dthr2);
            }
            lsum[qs] = lsum[qs] * alpha + sum;
#pragma unroll
            for (int db = 0; db < 4; ++db) o[qs][db] *= alpha;
        }
        const bf16* Vt = sm + b * LG_BUF + LG_KIMG;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16* v = Vt + (db * 16 + l15) * LG_VS + ks * 32 + 4 * g;
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(v);
                const bf16x4 hi = *reinterpret_cast<const bf16x4*>(v + 16);
                const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int qs = 0; qs < 2; ++qs) o[qs][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[qs][ks], o[qs][db], 0, 0, 0);
            }
        if (t + 1 < ntiles) store(b ^ 1, true);
        __syncthreads();
    }

    // bias variant: the head's multiplier (after softmax and dropout), 1 / (1 - p) of the dropout
    [[maybe_unused]] float hm = 1.f;
    if constexpr (MODE != 0) hm = p.head_mask ? p.head_mask[n * p.head_mask_sn + a] : 1.f;
    float inv[2];
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
        float l = lsum[qs];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        if constexpr (MODE != 0) inv[qs] = l > 0.f ? hm / l : 0.f;     // a row of -inf everywhere: context 0, probabilities 0
        else inv[qs] = 1.0f / l;
        const float oi = MODE == 2 ? inv[qs] * p.drop_keep : inv[qs];
        if (qrow[qs] < S) {
            bf16* c = (bf16*)p.ctx + ((int64_t)n * S + qrow[qs]) * H + a * 64 + 4 * g;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const bf16x4 w = {(bf16)(o[qs][db][0] * oi), (bf16)(o[qs][db][1] * oi), (bf16)(o[qs][db][2] * oi),
                                  (bf16)(o[qs][db][3] * oi)};
                *reinterpret_cast<bf16x4*>(c + db * 16) = w;
            }
        }
    }

    if constexpr (SIDE) {
        // second sweep: exact probabilities from the final row max and sum (K tiles only, one buffer)
        const int R = S - p.align_t, key0 = p.P + p.align_t;
        for (int t = 0; t < ntiles; ++t) {
            load(t, false);
            store(0, false);
            __syncthreads();
            if constexpr (MODE != 0) load_bias(t, bcur);
            f32x4 s[2][4];
            scores(t, 0, s, bcur);
#pragma unroll
            for (int qs = 0; qs < 2; ++qs) {
                const int q = qrow[qs];
                if (q >= S) continue;
                const float mf = (MODE != 0 && m[qs] == -INFINITY) ? 0.f : m[qs];
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    [[maybe_unused]] uint32_t wx = 0u, wy = 0u;     // the keep words of the lane's four keys of this block
                    if constexpr (MODE == 2) {
                        if (p.side_post_drop) {
                            wx = attn_drop_word(dbase[qs], 2 * (4 * t + kb), p.drop_key);
                            wy = attn_drop_word(dbase[qs], 2 * (4 * t + kb) + 1, p.drop_key);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = t * 64 + kb * 16 + 4 * g + i;
                        if (j >= L) continue;
                        float pr = __builtin_amdgcn_exp2f(s[qs][kb][i] - mf) * inv[qs];
                        if constexpr (MODE == 2) {
                            if (p.side_post_drop) pr = attn_keep_field(wx, wy, i, p.drop_thr16) ? pr * p.drop_keep : 0.f;
                        }
                        if (p.probs) p.probs[(((int64_t)n * p.A + a) * S + q) * L + j] = pr;
                        if (p.align_map && q < p.align_t && j >= key0)
                            atomicAdd(p.align_map + ((int64_t)n * p.align_t + q) * R + (j - key0), pr);
                    }
                }
            }
            __syncthreads();
        }
    }
}

// fp32 parity core: 4 waves x 16 queries per (64-query block, head, sequence); K and V tiles of 64 keys in LDS
template <bool BIAS, bool BITS = false>
__global__ __launch_bounds__(256) void attn_long_f32_kernel(AttnLongArgs p) {
    static_assert(!BITS || BIAS, "the binary variant reads its bits itself");
    __shared__ float sK[64 * 65], sV[64 * 65], sQ[4 * 16 * 64], sP[4 * 64];
    const int S = p.S, L = p.P + S, H = p.H;
    const int n = blockIdx.z, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntiles = (L + 63) >> 6;
    const float sc = 0.125f * LOG2E;
    const int q0 = blockIdx.x * 64 + wave * 16;
    float* q_img = sQ + wave * 16 * 64;
    float* p_img = sP + wave * 64;
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) {
        const int q = q0 + qi < S ? q0 + qi : S - 1;
        q_img[qi * 64 + lane] = ((const float*)p.qx)[((int64_t)n * S + q) * 3 * H + a * 64 + lane];
    }
    float m[16], lsum[16], o[16];
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) { m[qi] = -INFINITY; lsum[qi] = 0.f; o[qi] = 0.f; }

    auto load = [&](int t, bool with_v) {
        __syncthreads();
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, d = idx & 63, j = t * 64 + r;
            const float* row = j < L ? lg_row<float>(p, n, j) : nullptr;
            sK[r * 65 + d] = row ? row[H + a * 64 + d] : 0.f;
            if (with_v) sV[r * 65 + d] = row ? row[2 * H + a * 64 + d] : 0.f;
        }
        __syncthreads();
    };
    // log2-domain score of key t 64 + lane for query q0 + qi
    auto score = [&](int t, int qi) {
        const int j = t * 64 + lane;
        float s = 0.f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) s = fmaf(q_img[qi * 64 + d], sK[lane * 65 + d], s);
        const int q = q0 + qi < S ? q0 + qi : S - 1;
        if constexpr (BIAS) {
            if (j >= L) return -INFINITY;
            if constexpr (BITS) {                   // 0 / -10000 joins the bias before log2e: the folded call, bit for bit
                const bool see = (p.bits[((int64_t)n * S + q) * ((L + 31) >> 5) + (j >> 5)] >> (j & 31)) & 1u;
                const float bv = (p.bias ? p.bias[n * p.bias_sn + a * p.bias_sa + q * p.bias_sq + j] : 0.f) + (see ? 0.f : MODCR_NEG);
                return fmaf(s, sc, bv * LOG2E);
            }
            return p.bias ? fmaf(s, sc, p.bias[n * p.bias_sn + a * p.bias_sa + q * p.bias_sq + j] * LOG2E) : s * sc;
        } else {
            return j < L ? s * sc + lg_mask(p, n, q, j, L) : -INFINITY;
        }
    };
    // bias variant: keep factor (1 / (1 - p) or 0) of key t 64 + lane for query q0 + qi under the dropout of attn_common.h
    [[maybe_unused]] auto keep = [&](int t, int qi) {
        const int j = t * 64 + lane;
        uint32_t hx, hy;
        attn_drop_words(attn_drop_row(n, p.A, a, q0 + qi, L), j >> 2, p.drop_key, hx, hy);
        return attn_keep_field(hx, hy, j & 3, p.drop_thr16) ? p.drop_keep : 0.f;
    };

    for (int t = 0; t < ntiles; ++t) {
        load(t, true);
#pragma unroll
        for (int qi = 0; qi < 16; ++qi) {
            const float s = score(t, qi);
            const float mn = fmaxf(m[qi], wave_max(s));
            const float ms = (BIAS && mn == -INFINITY) ? 0.f : mn;     // every key so far at -inf: the tile contributes 0
            const float alpha = exp2f(m[qi] - ms);
            const float e = exp2f(s - ms);
            lsum[qi] = lsum[qi] * alpha + wave_sum(e);
            m[qi] = mn;
            if constexpr (BIAS) p_img[lane] = p.drop_thr16 ? e * keep(t, qi) : e;
            else p_img[lane] = e;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            float acc = 0.f;
#pragma unroll 8
            for (int j = 0; j < 64; ++j) acc = fmaf(p_img[j], sV[j * 65 + lane], acc);
            o[qi] = o[qi] * alpha + acc;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    [[maybe_unused]] float hm = 1.f;
    if constexpr (BIAS) hm = p.head_mask ? p.head_mask[n * p.head_mask_sn + a] : 1.f;
#pragma unroll
    for (int qi = 0; qi < 16; ++qi)
        if (q0 + qi < S) {
            float* c = (float*)p.ctx + ((int64_t)n * S + q0 + qi) * H + a * 64 + lane;
            if constexpr (BIAS) *c = lsum[qi] > 0.f ? o[qi] * hm / lsum[qi] : 0.f;     // a row of -inf everywhere: 0
            else *c = o[qi] / lsum[qi];
        }

    if (p.probs || p.align_map) {
        const int R = S - p.align_t, key0 = p.P + p.align_t;
        for (int t = 0; t < ntiles; ++t) {
            load(t, false);
#pragma unroll
            for (int qi = 0; qi < 16; ++qi) {
                const float s = score(t, qi);
                const int q = q0 + qi, j = t * 64 + lane;
                if (q >= S || j >= L) continue;
                float pr;
                if constexpr (BIAS) {
                    pr = lsum[qi] > 0.f ? exp2f(s - m[qi]) * hm / lsum[qi] : 0.f;
                    if (p.drop_thr16 && p.side_post_drop) pr *= keep(t, qi);
                } else {
                    pr = exp2f(s - m[qi]) / lsum[qi];
                }
                if (p.probs) p.probs[(((int64_t)n * p.A + a) * S + q) * L + j] = pr;
                if (p.align_map && q < p.align_t && j >= key0) atomicAdd(p.align_map + ((int64_t)n * p.align_t + q) * R + (j - key0), pr);
            }
        }
    }
}

template <typename K>
void lg_launch(K kernel, dim3 grid, dim3 block, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, const AttnLongArgs& p) {
    if (ev0 && ev1) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, ev0, ev1, 0, p);
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, p);
}

}  // namespace

int modcr_launch_attn_long(const AttnLongArgs& p, int32_t dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    const dim3 grid((p.S + 63) / 64, p.A, p.N);
    const bool side = p.probs || p.align_map;
    const bool bits = p.bits_on_bias && p.bits;     // (modcr_qkv_attn_long_align_fwd: the bits select the bias variant by themselves)
    const int mode = !(p.bias || p.head_mask || bits) ? 0 : p.drop_thr16 ? 2 : 1;
    if (dtype == MODCR_BF16) {
        if (bits) {
            if (mode == 1) {
                if (side) lg_launch(attn_long_bf16_kernel<true, 1, true>, grid, dim3(128), st, ev0, ev1, p);
                else lg_launch(attn_long_bf16_kernel<false, 1, true>, grid, dim3(128), st, ev0, ev1, p);
            } else {
                if (side) lg_launch(attn_long_bf16_kernel<true, 2, true>, grid, dim3(128), st, ev0, ev1, p);
                else lg_launch(attn_long_bf16_kernel<false, 2, true>, grid, dim3(128), st, ev0, ev1, p);
            }
        } else if (mode == 0) {
            if (side) lg_launch(attn_long_bf16_kernel<true, 0>, grid, dim3(128), st, ev0, ev1, p);
            else lg_launch(attn_long_bf16_kernel<false, 0>, grid, dim3(128), st, ev0, ev1, p);
        } else if (mode == 1) {
            if (side) lg_launch(attn_long_bf16_kernel<true, 1>, grid, dim3(128), st, ev0, ev1, p);
            else lg_launch(attn_long_bf16_kernel<false, 1>, grid, dim3(128), st, ev0, ev1, p);
        } else {
            if (side) lg_launch(attn_long_bf16_kernel<true, 2>, grid, dim3(128), st, ev0, ev1, p);
            else lg_launch(attn_long_bf16_kernel<false, 2>, grid, dim3(128), st, ev0, ev1, p);
        }
    } else if (mode == 0) {
        lg_launch(attn_long_f32_kernel<false>, grid, dim3(256), st, ev0, ev1, p);
    } else if (bits) {
        lg_launch((attn_long_f32_kernel<true, true>), grid, dim3(256), st, ev0, ev1, p);
    } else {
        lg_launch(attn_long_f32_kernel<true>, grid, dim3(256), st, ev0, ev1, p);
    }
    return modcr_check_launch(mode ? "attn_bias" : "attn_long");
}
