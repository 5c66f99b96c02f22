// Streaming attention core backward (CDNA4 / gfx950; head size 64): the arithmetic of attn_bias_bwd.hip -- additive fp32 bias, head
// mask, prefix rows, gradient of the head mask -- for S queries against 256 < L = P + S <= 512 keys, where a head's key row no longer
// fits LDS.  Attention-probability dropout in the DROP instantiations (modcr_qkv_attn_long_drop_bwd): the wide counter layout of
// attn_common.h (row stride 512), regenerated in both kernels, never stored; see "Dropout" below.  Per (sequence n, head a), keys
// j < P are the prefix rows, keys j >= P the sequence's own rows:
//     s_ij = q_i.k_j / 8 + bias[n, a, i, j]     P = softmax_j(s)     ctx = hm[n, a] P.V
//     dV = hm P^T.dctx     dP = hm (dctx.V^T)     dS = P o (dP - rowsum(dP o P))
//     dQ = dS.K / 8  [S rows]     dK = dS^T.Q / 8  [L rows]     d_bias = dS  [N, A, S, L]     d_hm[n, a] = sum_i dctx_i . (P.V)_i
// The rows stream through LDS in tiles of 64, double-buffered (the next tile waits in registers under the current one's arithmetic,
// as in attn_long.hip).  Two launches over (64-row block, head, sequence) and a third, tiny one:
//   query kernel, per 64-QUERY block, two sweeps over the key tiles
//     sweep 1 (statistics): the forward core's online softmax with its context accumulators; leaves per query row, fp32, in the
//              workspace (b.stats [N A][3][SP], SP = S rounded up to 64): the row max (log2 domain, -inf replaced by 0), 1 / row sum
//              (1 / 0 replaced by 0) and D_i = dctx_i . (P.V)_i -- formed WITHOUT hm;
//     sweep 2 (query pass): s recomputed, P = exp2(s - max) / sum, dP, dS' = P o (dP - D); d_bias tile = hm dS'; dQ += dS'.K, stored as
//              hm dQ / 8;
//   key kernel, per 64-KEY block, streaming the query tiles (Q | dO rows) with the statistics: the same quantities with the key on
//              the lane; dV += P^T.dO, dK += dS'^T.Q; stored as hm dV, hm dK / 8 -- keys j < P to the prefix gradient rows, the rest
//              to the own rows' dq | dk | dv;
//   d_head_mask[n, a] = sum_i D_i: one wave per (n, a), a fixed order (rows 64 r + lane ascending, then the butterfly).
// hm is a common factor of dP and of delta = hm D, hence of every result: the arithmetic runs with hm = 1 and hm enters at the stores
// (attn_bias_bwd.hip's rule), so hm = 0 makes dQ, dK, dV and d_bias exactly 0 while d_hm keeps its value.
// Every output element is written by exactly one lane; nothing is accumulated across workgroups: no atomics, two calls are
// bit-identical.  Conventions of the other cores: keys beyond L carry -inf; a single -inf entry is probability 0 and d_bias 0; a
// query row whose every key is -inf has P = 0 and adds exactly nothing; rows past S (queries) or L (keys) are never stored, their
// images are zeros and a padded query takes the bias of row S - 1 in both kernels, so its probabilities are finite and consistent.
// The bias is read through its strides, never expanded: in the query kernel a lane's four keys are consecutive floats (one 16-byte
// load when the address is aligned and the four keys are inside the row, scalar loads otherwise); in the key kernel a lane's four
// values are four query rows of one key.
//
// bf16 core (core 3): 4 waves x 16 rows per workgroup, v_mfma_f32_16x16x32_bf16 with attn_long.hip's fragment layouts (S^T = K.Q^T,
// the streamed row on the MFMA's row side, the owned row on the lane; accumulators become operands as bf16), row images of 128-byte
// rows under swz128 read row-wise (ds_read_b128) and transposed (abb_tr8).  As in the forward above 256 keys the q rows are NOT
// pre-scaled: the accumulator takes log2e / 8.
// fp32 core (core 4): the same tiling with VALU products; the streamed row on the lane for the scores, the feature on the lane for
// the accumulators.  fp32 rows and fp32 dctx: the host sends every bf16 call above 256 keys to core 3.
//
// Dropout (template parameter DROP; the instantiations without it compile as before): with m the forward's keep mask and
// P~ = P o m / (1 - p),   ctx = hm P~.V,   D_i = dctx_i . (P~.V)_i,   dP = (dctx.V^T) o m / (1 - p),   dS' = P o (dP - D),   dV = P~^T.dO.
//   query kernel: the query lies on the lane and its g is the layout's l4, so one hash base per lane serves both sweeps; sweep 1
//     clears the dropped bf16 pairs of the P^T fragments as the forward does (attn_drop8_rt; the row sum keeps the un-dropped
//     weights) and D takes 1 / (1 - p); sweep 2 multiplies dP by keep / (1 - p) from the two words of each 16-key block.
//   key kernel: the key lies on the lane, its four values are four QUERIES -- four counter rows, but one l4 and one pair of word
//     multipliers, fixed for the whole kernel.  Each lane of a quad hashes the row of one of the quad's four queries and the words
//     travel by quad broadcasts (attn_bias_bwd_mfma_kernel's scheme): three multiply-folds per lane and 16-query block.
//
// Dense mask bits and the align map's gradient (template parameters MASK and DALIGN, modcr_qkv_attn_long_align_bwd, P = 0; the
// instantiations without them compile as before):
//   MASK: bit j of bits[n, i, :] clear adds -10000 to the bias of (i, j) before the multiplication by log2e, as the forward's BITS
//     variant does; the query kernel loads the two words of a tile and query, the key kernel one word per query row and picks the
//     lane's bit.  A padded query row takes row S - 1's words in both kernels.
//   DALIGN: G = d_align [N, T, R] is the gradient of align_map[n, i, r] = sum_a hm A^side_{i, T + r} (i < T), A^side = P, or P~ with
//     side_post_drop.  E_ij = G[n, i, j - T] for i < T <= j, else 0:
//         dP_ij = (dctx_i . v_j) m_ij / (1 - p) + E_ij (post ? m_ij / (1 - p) : 1)        D_i = dctx_i . (P~.V)_i + sum_j A^side_ij E_ij
//     The align share of D_i is one more online accumulator of sweep 1: c_i = sum_j e_ij E_ij (keep factor), e_ij the tile's
//     exponentials, rescaled by the running max's alpha like the row sum, reduced over the row's four lanes and divided by the row sum
//     at the end -- no pass of its own.  It is skipped for query blocks at or beyond T and key tiles below T (both uniform); sweep 2
//     and the key kernel add E to dP.  A lane's four E values are consecutive floats in the query kernel (one 16-byte load when the
//     address is aligned and the four are inside the row, scalar loads otherwise) and four query rows of one key, R floats apart, in
//     the key kernel.  hm stays a common factor (the map carries it too), so d_hm = sum_i D_i with both shares.
#include "common.h"
#include "attn_common.h"

namespace {

struct ALB {
    static constexpr int NT = 256;                          // 4 waves x 16 rows
    static constexpr int IMG = 64 * 128;                    // 64 rows x [64] bf16, swz128
    static constexpr int BUF = 2 * IMG;                     // query kernel: K | V    key kernel: Q | dO
    static constexpr int SMEM = 2 * BUF;                    // double-buffered: 32 KB
    // fp32 core: two [64][65] tiles, two per-wave [16][64] row sets, per-wave scratch rows, the tile's statistics
    static constexpr int F32_Q = (2 * 64 * 65 + 2 * 4 * 16 * 64 + 4 * 64) * 4;
    static constexpr int F32_K = (2 * 64 * 65 + 2 * 4 * 16 * 64 + 2 * 4 * 64 + 3 * 64) * 4;
};

__device__ __forceinline__ bf16x8 alb_zero8() {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16)0.f;
    return o;
}

// the lane's four bias values bias_row[j .. j + 3] (keys beyond L: 0, they are overwritten with -inf)
__device__ __forceinline__ f32x4 alb_bias4(const float* row, bool vec, int j, int L) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && j + 3 < L) return *reinterpret_cast<const f32x4*>(row + j);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (j + i < L) v[i] = row[j + i];
    return v;
}

// the lane's four align-map gradients grow[jr .. jr + 3] of one text row (jr = key - T; outside [0, R): 0)
__device__ __forceinline__ f32x4 alb_dalign4(const float* grow, int jr, int R) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (jr >= 0 && jr + 3 < R && (reinterpret_cast<uintptr_t>(grow + jr) & 15) == 0) return *reinterpret_cast<const f32x4*>(grow + jr);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (jr + i >= 0 && jr + i < R) v[i] = grow[jr + i];
    return v;
}

// ---- bf16 core, query kernel: statistics sweep + query sweep of one 64-query block -----------------------------------------
template <bool BIAS, bool DBIAS, bool DROP, bool MASK = false, bool DALIGN = false>
__global__ __launch_bounds__(256) void attn_long_bwd_q_kernel(AttnBiasBwdArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[ALB::SMEM];
    const int S = p.S, P = p.P, L = S + P, H = p.H;
    const int n = blockIdx.z, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int ntiles = (L + 63) >> 6, SP = (S + 63) & ~63;
    const bf16* qkv = reinterpret_cast<const bf16*>(p.qkv) + (int64_t)n * S * 3 * H + a * 64;      // own rows: q | k | v
    const bf16* kvh = reinterpret_cast<const bf16*>(p.kvh) + (int64_t)n * P * 2 * H + a * 64;      // prefix rows: k | v
    const bf16* dctx = reinterpret_cast<const bf16*>(p.dctx) + (int64_t)n * S * H + a * 64;
    float* stats = p.stats + ((int64_t)n * p.A + a) * 3 * SP;
    constexpr float SC = 0.125f * LOG2E;
    const float hm = p.head_mask ? p.head_mask[(int64_t)n * p.head_mask_sn + a] : 1.0f;

    // the lane's query: Q and dO fragments (B operands), zeros beyond S; such a row takes the bias of row S - 1
    const int qrow = blockIdx.x * 64 + wave * 16 + l15;
    const int qc = min(qrow, S - 1);
    bf16x8 qf[2], fdo[2];
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
        qf[ds] = qrow < S ? *reinterpret_cast<const bf16x8*>(qkv + (int64_t)qrow * 3 * H + 32 * ds + 8 * g) : alb_zero8();
        fdo[ds] = qrow < S ? *reinterpret_cast<const bf16x8*>(dctx + (int64_t)qrow * H + 32 * ds + 8 * g) : alb_zero8();
    }
    [[maybe_unused]] const float* brow = nullptr;
    [[maybe_unused]] bool bvec = false;
    if constexpr (BIAS) {
        brow = p.bias + (int64_t)n * p.bias_sn + (int64_t)a * p.bias_sa + (int64_t)qc * p.bias_sq;
        bvec = (reinterpret_cast<uintptr_t>(brow) & 15) == 0;
    }

    // dropout: the lane's hash base (its g is the layout's l4; the wide layout: L > 256), the packed threshold
    [[maybe_unused]] uint32_t dbase = 0u, dthr2 = 0u;
    if constexpr (DROP) {
        dbase = attn_drop_base(attn_drop_row(n, p.A, a, qrow, L), (uint32_t)g, p.drop_key);
        dthr2 = attn_thrm1_2(p.drop_thr16);
    }

    // MASK: the query's row of words (P = 0: L = S keys).  DALIGN: the query's row of G; text rows only, in blocks that hold one
    [[maybe_unused]] const uint32_t* wrow = nullptr;
    [[maybe_unused]] const int LW = (L + 31) >> 5;
    if constexpr (MASK) wrow = p.bits + ((int64_t)n * S + qc) * LW;
    [[maybe_unused]] const int T = DALIGN ? p.align_t : 0, R = S - T;
    [[maybe_unused]] const bool ablock = DALIGN && (int)blockIdx.x * 64 < T;
    [[maybe_unused]] const float* grow = nullptr;
    if constexpr (DALIGN) grow = p.d_align + ((int64_t)n * T + min(qrow, T - 1)) * R;
    [[maybe_unused]] const bool apost = DALIGN && DROP && p.side_post_drop;
    // E (x the keep factor when the map took the dropped probabilities) of the lane's four keys of block kb of tile t
    [[maybe_unused]] auto align4 = [&](int t, int kb) {
        f32x4 e4 = alb_dalign4(grow, t * 64 + kb * 16 + 4 * g - T, R);
        if (qrow >= T) e4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (DROP) {
            if (apost) {
                const uint32_t hx = attn_drop_word(dbase, 2 * (4 * t + kb), p.drop_key);
                const uint32_t hy = attn_drop_word(dbase, 2 * (4 * t + kb) + 1, p.drop_key);
#pragma unroll
                for (int i = 0; i < 4; ++i) e4[i] = attn_keep_field(hx, hy, i, p.drop_thr16) ? e4[i] * p.drop_keep : 0.f;
            }
        }
        return e4;
    };

    // staging: piece r of thread t = row (t + 256 r) >> 3 of the tile, 16-byte chunk t & 7; zeros beyond L
    bf16x8 kreg[2], vreg[2];
    auto load = [&](int t) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = t * 64 + ((tid + 256 * r) >> 3), c = tid & 7;
            if (j < L) {
                const bf16* row = j < P ? kvh + (int64_t)j * 2 * H : qkv + (int64_t)(j - P) * 3 * H + H;
                kreg[r] = *reinterpret_cast<const bf16x8*>(row + c * 8);
                vreg[r] = *reinterpret_cast<const bf16x8*>(row + H + c * 8);
            } else {
                kreg[r] = alb_zero8();
                vreg[r] = alb_zero8();
            }
        }
    };
    auto store = [&](int b) {
        unsigned char* K = smem + b * ALB::BUF;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int off = swz128((tid + 256 * r) >> 3, tid & 7);
            *reinterpret_cast<bf16x8*>(K + off) = kreg[r];
            *reinterpret_cast<bf16x8*>(K + ALB::IMG + off) = vreg[r];
        }
    };
    // log2-domain scores of tile t (buffer b): s[kb][i] = key 64 t + 16 kb + 4 g + i, query qrow
    auto scores = [&](int t, int b, f32x4 (&s)[4]) {
        const unsigned char* K = smem + b * ALB::BUF;
        [[maybe_unused]] f32x4 bb[4];
        if constexpr (BIAS) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) bb[kb] = alb_bias4(brow, bvec, t * 64 + kb * 16 + 4 * g, L);
        }
        [[maybe_unused]] uint32_t wb[2];                    // MASK: the tile's two 32-key words of the query
        if constexpr (MASK) {
            wb[0] = wrow[2 * t];
            wb[1] = 2 * t + 1 < LW ? wrow[2 * t + 1] : 0u;
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(K + swz128(kb * 16 + l15, g));
            const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(K + swz128(kb * 16 + l15, 4 + g));
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], c, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool in = t * 64 + kb * 16 + 4 * g + i < L;
                if constexpr (MASK) {                       // 0 / -10000 joins the bias before log2e, as in the forward
                    const float hide = ((wb[kb >> 1] >> ((kb & 1) * 16 + 4 * g + i)) & 1u) ? 0.f : MODCR_NEG;
                    s[kb][i] = in ? fmaf(c[i], SC, (BIAS ? bb[kb][i] + hide : hide) * LOG2E) : -INFINITY;
                } else if constexpr (BIAS) s[kb][i] = in ? fmaf(c[i], SC, bb[kb][i] * LOG2E) : -INFINITY;
                else s[kb][i] = in ? c[i] * SC : -INFINITY;
            }
        }
    };
    // one sweep over the key tiles: tile t + 1 is requested before body(t) and stored behind it
    auto sweep = [&](auto&& body) {
        load(0);
        store(0);
        __syncthreads();
        for (int t = 0; t < ntiles; ++t) {
            const int b = t & 1;
            if (t + 1 < ntiles) load(t + 1);
            body(t, b);
            if (t + 1 < ntiles) store(b ^ 1);
            __syncthreads();
        }
    };

    // ---- sweep 1: row max, row sum, context accumulators (online softmax) ------------------------------------------
    float m = -INFINITY, lsum = 0.f;
    [[maybe_unused]] float asum = 0.f;                      // DALIGN: sum_j e_ij E_ij (keep factor), on the row sum's scale
    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    sweep([&](int t, int b) {
        f32x4 s[4];
        scores(t, b, s);
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[kb][i]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float ms = mn == -INFINITY ? 0.f : mn;        // every key so far at -inf: exponentials against 0, all of them 0
        const float alpha = __builtin_amdgcn_exp2f(m - ms);
        m = mn;
        float sum = 0.f;
        [[maybe_unused]] float asub = 0.f;
        [[maybe_unused]] const bool atile = ablock && t * 64 + 63 >= T;       // (uniform: the block holds text rows, the tile region keys)
        bf16x8 pb[2];                                       // P^T fragments: step ks = keys 32 ks + (4 g + e | 16 + 4 g + e)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            [[maybe_unused]] f32x4 e4 = {0.f, 0.f, 0.f, 0.f};
            if constexpr (DALIGN) {
                if (atile) e4 = align4(t, kb);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = __builtin_amdgcn_exp2f(s[kb][i] - ms);
                sum += e;
                if constexpr (DALIGN) asub = fmaf(e, e4[i], asub);
                pb[kb >> 1][(kb & 1) * 4 + i] = (bf16)e;
            }
        }
        if constexpr (DALIGN) asum = asum * alpha + asub;
        if constexpr (DROP) {                               // the row sum keeps the un-dropped weights; the context takes P o m
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) pb[ks] = attn_drop8_rt(pb[ks], dbase, 2 * t + ks, p.drop_key, dthr2);
        }
        lsum = lsum * alpha + sum;
        const unsigned char* V = smem + b * ALB::BUF + ALB::IMG;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            o[db] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abb_tr8(V, ks * 32, db, l15, g), pb[ks], o[db], 0, 0, 0);
        }
    });
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;       // a row of -inf everywhere: probabilities 0, not 0 / 0
    const float mf = m == -INFINITY ? 0.f : m;
    // D = dctx . (P.V): o[db][i] is feature 16 db + 4 g + i of the query's unnormalised context
    float dl = 0.f;
    if (qrow < S) {
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const bf16x4 d4 = *reinterpret_cast<const bf16x4*>(dctx + (int64_t)qrow * H + db * 16 + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) dl = fmaf(o[db][i], (float)d4[i], dl);
        }
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    dl *= DROP ? inv * p.drop_keep : inv;
    if constexpr (DALIGN) {                                 // the align share of D: the accumulator over the row's four lanes / row sum
        asum += __shfl_xor(asum, 16, 64);
        asum += __shfl_xor(asum, 32, 64);
        dl = fmaf(asum, inv, dl);
    }
    if (g == 0) { stats[qrow] = mf; stats[SP + qrow] = inv; stats[2 * SP + qrow] = dl; }

    // ---- sweep 2: dS, d_bias, dQ ------------------------------------------------------------------------------------
    f32x4 dq[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) dq[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] float* drow = nullptr;
    [[maybe_unused]] bool dvec = false;
    if constexpr (DBIAS) {
        drow = p.d_bias + (((int64_t)n * p.A + a) * S + qc) * L;
        dvec = (reinterpret_cast<uintptr_t>(drow) & 15) == 0;
    }
    sweep([&](int t, int b) {
        f32x4 s[4];
        scores(t, b, s);
        const unsigned char* K = smem + b * ALB::BUF;
        const unsigned char* V = K + ALB::IMG;
        bf16x8 dsb[2];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(V + swz128(kb * 16 + l15, g));
            const bf16x8 v1 = *reinterpret_cast<const bf16x8*>(V + swz128(kb * 16 + l15, 4 + g));
            f32x4 dp = {0.f, 0.f, 0.f, 0.f};
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, fdo[0], dp, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, fdo[1], dp, 0, 0, 0);
            if constexpr (DROP) {                           // dP = (dctx.V^T) o m / (1 - p): the two words of this 16-key block
                const uint32_t hx = attn_drop_word(dbase, 2 * (4 * t + kb), p.drop_key);
                const uint32_t hy = attn_drop_word(dbase, 2 * (4 * t + kb) + 1, p.drop_key);
#pragma unroll
                for (int i = 0; i < 4; ++i) dp[i] = attn_keep_field(hx, hy, i, p.drop_thr16) ? dp[i] * p.drop_keep : 0.f;
            }
            if constexpr (DALIGN) {                         // + E, under the keep mask when the map took the dropped probabilities
                if (ablock && t * 64 + 63 >= T) dp += align4(t, kb);
            }
            f32x4 ds;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ds[i] = __builtin_amdgcn_exp2f(s[kb][i] - mf) * inv * (dp[i] - dl);
                dsb[kb >> 1][(kb & 1) * 4 + i] = (bf16)ds[i];
            }
            if constexpr (DBIAS) {
                const int j = t * 64 + kb * 16 + 4 * g;
                if (qrow < S) {
                    if (dvec && j + 3 < L) *reinterpret_cast<f32x4*>(drow + j) = ds * hm;
                    else
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (j + i < L) drow[j + i] = ds[i] * hm;
                }
            }
        }
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) dq[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abb_tr8(K, ks * 32, db, l15, g), dsb[ks], dq[db], 0, 0, 0);
    });
    if (qrow < S) {
        const float qscale = 0.125f * hm;
        bf16* oq = reinterpret_cast<bf16*>(p.dqkv) + ((int64_t)n * S + qrow) * 3 * H + a * 64 + 4 * g;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const f32x4 v = dq[db];
            *reinterpret_cast<bf16x4*>(oq + db * 16) = bf16x4{(bf16)(v[0] * qscale), (bf16)(v[1] * qscale), (bf16)(v[2] * qscale), (bf16)(v[3] * qscale)};
        }
    }
}

// ---- bf16 core, key kernel: dK | dV of one 64-key block over the streamed query tiles ----------------------------------------
// (DALIGN without DROP: asked to stay inside the two waves per SIMD its twins have -- 218-253 registers, no spill; with DROP the same
// request spills 7-30 registers, so those are left alone: 252-292 registers, three of the four at one wave per SIMD)
template <bool BIAS, bool DROP, bool MASK = false, bool DALIGN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DALIGN && !DROP ? 2 : 1))) void attn_long_bwd_k_kernel(AttnBiasBwdArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[ALB::SMEM];
    const int S = p.S, P = p.P, L = S + P, H = p.H;
    const int n = blockIdx.z, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int qtiles = (S + 63) >> 6, SP = qtiles * 64;
    const bf16* qkv = reinterpret_cast<const bf16*>(p.qkv) + (int64_t)n * S * 3 * H + a * 64;
    const bf16* kvh = reinterpret_cast<const bf16*>(p.kvh) + (int64_t)n * P * 2 * H + a * 64;
    const bf16* dctx = reinterpret_cast<const bf16*>(p.dctx) + (int64_t)n * S * H + a * 64;
    const float* stats = p.stats + ((int64_t)n * p.A + a) * 3 * SP;
    [[maybe_unused]] const float* bias = BIAS ? p.bias + (int64_t)n * p.bias_sn + (int64_t)a * p.bias_sa : nullptr;
    [[maybe_unused]] const uint32_t bsq = (uint32_t)p.bias_sq;
    constexpr float SC = 0.125f * LOG2E;
    const float hm = p.head_mask ? p.head_mask[(int64_t)n * p.head_mask_sn + a] : 1.0f;

    // the lane's key: K and V fragments (B operands); a key beyond L reads row L - 1 and carries -inf
    const int key = blockIdx.x * 64 + wave * 16 + l15;
    const int keyc = min(key, L - 1);
    const float kpad = key < L ? 0.f : -INFINITY;
    bf16x8 fkk[2], fvv[2];
    {
        const bf16* row = keyc < P ? kvh + (int64_t)keyc * 2 * H : qkv + (int64_t)(keyc - P) * 3 * H + H;
#pragma unroll
        for (int ds = 0; ds < 2; ++ds) {
            fkk[ds] = *reinterpret_cast<const bf16x8*>(row + 32 * ds + 8 * g);
            fvv[ds] = *reinterpret_cast<const bf16x8*>(row + H + 32 * ds + 8 * g);
        }
    }
    // dropout: what the lane's key fixes for the whole kernel -- its l4, the multipliers of its 16-key block's two words -- and the
    // counter row of query 0 of this (sequence, head); the lane hashes query q0 + (l15 & 3) of its quad's four
    [[maybe_unused]] uint32_t drow0 = 0u, dl4 = 0u, dcx = 0u, dcy = 0u;
    if constexpr (DROP) {
        drow0 = attn_drop_row(n, p.A, a, l15 & 3, L);
        dl4 = (uint32_t)(key >> 2) & 3u;
        dcx = attn_drop_const(2 * (key >> 4));
        dcy = attn_drop_const(2 * (key >> 4) + 1);
    }
    // MASK: the key's word column and bit (P = 0: L = S).  DALIGN: the key's column of G; region keys only, in blocks that hold one
    [[maybe_unused]] const int LW = (L + 31) >> 5;
    [[maybe_unused]] const uint32_t* wcol = nullptr;
    if constexpr (MASK) wcol = p.bits + (int64_t)n * S * LW + (keyc >> 5);
    [[maybe_unused]] const int T = DALIGN ? p.align_t : 0, R = S - T;
    [[maybe_unused]] const bool ablock = DALIGN && (int)blockIdx.x * 64 + 63 >= T;
    [[maybe_unused]] const bool akey = DALIGN && key >= T && key < L;
    [[maybe_unused]] const float* gcol = nullptr;
    if constexpr (DALIGN) gcol = p.d_align + (int64_t)n * T * R + (akey ? key - T : 0);
    [[maybe_unused]] const bool apost = DALIGN && DROP && p.side_post_drop;
    // staging of query tile t: Q | dO rows, zeros beyond S
    bf16x8 qreg[2], dreg[2];
    auto load = [&](int t) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = t * 64 + ((tid + 256 * r) >> 3), c = tid & 7;
            qreg[r] = i < S ? *reinterpret_cast<const bf16x8*>(qkv + (int64_t)i * 3 * H + c * 8) : alb_zero8();
            dreg[r] = i < S ? *reinterpret_cast<const bf16x8*>(dctx + (int64_t)i * H + c * 8) : alb_zero8();
        }
    };
    auto store = [&](int b) {
        unsigned char* Q = smem + b * ALB::BUF;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int off = swz128((tid + 256 * r) >> 3, tid & 7);
            *reinterpret_cast<bf16x8*>(Q + off) = qreg[r];
            *reinterpret_cast<bf16x8*>(Q + ALB::IMG + off) = dreg[r];
        }
    };
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) { dk[db] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    load(0);
    store(0);
    __syncthreads();
    for (int t = 0; t < qtiles; ++t) {
        const int b = t & 1;
        if (t + 1 < qtiles) load(t + 1);
        const unsigned char* Q = smem + b * ALB::BUF;
        const unsigned char* D = Q + ALB::IMG;
        bf16x8 pB[2], dsB[2];                               // fragments over the tile's queries 32 ks + (4 g + e | 16 + 4 g + e)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
            const int q0 = t * 64 + qb * 16 + 4 * g;        // the lane's four queries q0 .. q0 + 3 (< SP)
            const f32x4 m4 = *reinterpret_cast<const f32x4*>(stats + q0);
            const f32x4 i4 = *reinterpret_cast<const f32x4*>(stats + SP + q0);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(stats + 2 * SP + q0);
            [[maybe_unused]] f32x4 bq;
            if constexpr (BIAS) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bq[e] = bias[(uint32_t)min(q0 + e, S - 1) * bsq + (uint32_t)keyc];
            }
            [[maybe_unused]] f32x4 hide;                    // MASK: 0 / -10000 of (query q0 + e, key): one word per query row, the lane's bit
            if constexpr (MASK) {
#pragma unroll
                for (int e = 0; e < 4; ++e) hide[e] = ((wcol[(uint32_t)min(q0 + e, S - 1) * (uint32_t)LW] >> (keyc & 31)) & 1u) ? 0.f : MODCR_NEG;
            }
            [[maybe_unused]] f32x4 e4 = {0.f, 0.f, 0.f, 0.f};   // DALIGN: E of the lane's four queries, R floats apart (text rows, region key)
            if constexpr (DALIGN) {
                if (ablock && t * 64 < T) {                 // (uniform: the block holds region keys, the tile text rows)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (akey && q0 + e < T) e4[e] = gcol[(uint32_t)(q0 + e) * (uint32_t)R];
                }
            }
            const bf16x8 fq0 = *reinterpret_cast<const bf16x8*>(Q + swz128(qb * 16 + l15, g));
            const bf16x8 fq1 = *reinterpret_cast<const bf16x8*>(Q + swz128(qb * 16 + l15, 4 + g));
            const bf16x8 fd0 = *reinterpret_cast<const bf16x8*>(D + swz128(qb * 16 + l15, g));
            const bf16x8 fd1 = *reinterpret_cast<const bf16x8*>(D + swz128(qb * 16 + l15, 4 + g));
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq0, fkk[0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq1, fkk[1], c, 0, 0, 0);
            f32x4 dp = {0.f, 0.f, 0.f, 0.f};
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd0, fvv[0], dp, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd1, fvv[1], dp, 0, 0, 0);
            // dropout: the lane's four values are four queries of ONE key, four counter rows; each lane of a quad hashes one of them
            // (both words of the key's 16-key block) and quad broadcasts hand them round
            [[maybe_unused]] uint32_t xq[4], yq[4];
            if constexpr (DROP) {
                const uint32_t hb = attn_drop_base(drow0 + (uint32_t)q0, dl4, p.drop_key);
                const uint32_t hqx = attn_drop_fold(hb, dcx, p.drop_key), hqy = attn_drop_fold(hb, dcy, p.drop_key);
                xq[0] = quad_bcast<0>(hqx); xq[1] = quad_bcast<1>(hqx); xq[2] = quad_bcast<2>(hqx); xq[3] = quad_bcast<3>(hqx);
                yq[0] = quad_bcast<0>(hqy); yq[1] = quad_bcast<1>(hqy); yq[2] = quad_bcast<2>(hqy); yq[3] = quad_bcast<3>(hqy);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float sv;
                if constexpr (MASK) sv = fmaf(c[e], SC, (BIAS ? bq[e] + hide[e] : hide[e]) * LOG2E) + kpad;
                else sv = (BIAS ? fmaf(c[e], SC, bq[e] * LOG2E) : c[e] * SC) + kpad;
                const float pe = __builtin_amdgcn_exp2f(sv - m4[e]) * i4[e];
                if constexpr (DROP) {
                    const float mk = attn_keep_field(xq[e], yq[e], key & 3, p.drop_thr16) ? p.drop_keep : 0.f;   // of (query q0 + e, key)
                    pB[qb >> 1][(qb & 1) * 4 + e] = (bf16)(pe * mk);        // dV takes the masked probabilities
                    if constexpr (DALIGN) dsB[qb >> 1][(qb & 1) * 4 + e] = (bf16)(pe * ((apost ? mk * (dp[e] + e4[e]) : fmaf(mk, dp[e], e4[e])) - d4[e]));
                    else dsB[qb >> 1][(qb & 1) * 4 + e] = (bf16)(pe * (mk * dp[e] - d4[e]));
                } else {
                    pB[qb >> 1][(qb & 1) * 4 + e] = (bf16)pe;
                    if constexpr (DALIGN) dsB[qb >> 1][(qb & 1) * 4 + e] = (bf16)(pe * (dp[e] + e4[e] - d4[e]));
                    else dsB[qb >> 1][(qb & 1) * 4 + e] = (bf16)(pe * (dp[e] - d4[e]));
                }
            }
        }
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                dv[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abb_tr8(D, ks * 32, db, l15, g), pB[ks], dv[db], 0, 0, 0);
                dk[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(abb_tr8(Q, ks * 32, db, l15, g), dsB[ks], dk[db], 0, 0, 0);
            }
        if (t + 1 < qtiles) store(b ^ 1);
        __syncthreads();
    }
    if (key < L) {
        bf16* ob = key < P ? reinterpret_cast<bf16*>(p.dkvh) + ((int64_t)n * P + key) * 2 * H
                           : reinterpret_cast<bf16*>(p.dqkv) + ((int64_t)n * S + (key - P)) * 3 * H + H;
        ob += a * 64 + 4 * g;
        const float kscale = 0.125f * hm;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const f32x4 ok = dk[db], ov = dv[db];
            *reinterpret_cast<bf16x4*>(ob + db * 16) = bf16x4{(bf16)(ok[0] * kscale), (bf16)(ok[1] * kscale), (bf16)(ok[2] * kscale), (bf16)(ok[3] * kscale)};
            *reinterpret_cast<bf16x4*>(ob + H + db * 16) = bf16x4{(bf16)(ov[0] * hm), (bf16)(ov[1] * hm), (bf16)(ov[2] * hm), (bf16)(ov[3] * hm)};
        }
    }
}

// ---- d_head_mask[n, a] = sum over the S query rows of D: one wave per (n, a), a fixed order ---------------------------------
__global__ __launch_bounds__(64) void attn_long_bwd_dhm_kernel(const float* stats, float* d_head_mask, int S, int SP) {
    const float* D = stats + ((int64_t)blockIdx.x * 3 + 2) * SP;
    const int lane = threadIdx.x;
    float gsum = 0.f;
    for (int i = lane; i < S; i += 64) gsum += D[i];
    gsum = wave_sum(gsum);
    if (lane == 0) d_head_mask[blockIdx.x] = gsum;
}

// ---- exact fp32 core, query kernel: 4 waves x 16 queries; K, V tiles of 64 keys in LDS ----------------------------------------
template <bool DROP, bool MASK = false, bool DALIGN = false>
__global__ __launch_bounds__(256) void attn_long_bwd_q_f32_kernel(AttnBiasBwdArgs p) {
    extern __shared__ float sm[];
    float* sK = sm;                          // [64][65]
    float* sV = sK + 64 * 65;                // [64][65]
    float* sQ = sV + 64 * 65;                // per wave [16][64]: the wave's query rows
    float* sD = sQ + 4 * 16 * 64;            // per wave [16][64]: their dO rows
    float* sP = sD + 4 * 16 * 64;            // per wave [64]
    const int S = p.S, P = p.P, L = S + P, H = p.H;
    const int n = blockIdx.z, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntiles = (L + 63) >> 6, SP = (S + 63) & ~63;
    constexpr float SC = 0.125f * LOG2E;
    const float* qkv = reinterpret_cast<const float*>(p.qkv) + (int64_t)n * S * 3 * H + a * 64;
    const float* kvh = reinterpret_cast<const float*>(p.kvh) + (int64_t)n * P * 2 * H + a * 64;
    const float* dctx = reinterpret_cast<const float*>(p.dctx) + (int64_t)n * S * H + a * 64;
    const float* bias = p.bias ? p.bias + (int64_t)n * p.bias_sn + (int64_t)a * p.bias_sa : nullptr;
    float* dbias = p.d_bias ? p.d_bias + ((int64_t)n * p.A + a) * S * L : nullptr;
    float* stats = p.stats + ((int64_t)n * p.A + a) * 3 * SP;
    const float hm = p.head_mask ? p.head_mask[(int64_t)n * p.head_mask_sn + a] : 1.0f;
    const int q0 = blockIdx.x * 64 + wave * 16;
    float* q_img = sQ + wave * 16 * 64;
    float* d_img = sD + wave * 16 * 64;
    float* p_img = sP + wave * 64;
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) {        // zeros beyond S
        const int q = q0 + qi;
        q_img[qi * 64 + lane] = q < S ? qkv[(int64_t)q * 3 * H + lane] : 0.f;
        d_img[qi * 64 + lane] = q < S ? dctx[(int64_t)q * H + lane] : 0.f;
    }
    auto load = [&](int t) {
        __syncthreads();
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, d = idx & 63, j = t * 64 + r;
            const float* row = j >= L ? nullptr : j < P ? kvh + (int64_t)j * 2 * H : qkv + (int64_t)(j - P) * 3 * H + H;
            sK[r * 65 + d] = row ? row[d] : 0.f;
            sV[r * 65 + d] = row ? row[H + d] : 0.f;
        }
        __syncthreads();
    };
    // log2-domain score of key 64 t + lane for query q0 + qi (a padded query takes the bias of row S - 1)
    auto score = [&](int t, int qi) {
        const int j = t * 64 + lane;
        if (j >= L) return -INFINITY;
        float s = 0.f;
#pragma unroll 8
        for (int d = 0; d < 64; ++d) s = fmaf(q_img[qi * 64 + d], sK[lane * 65 + d], s);
        const int q = min(q0 + qi, S - 1);
        if constexpr (MASK) {                   // 0 / -10000 joins the bias before log2e, as in the forward
            const bool see = (p.bits[((int64_t)n * S + q) * ((L + 31) >> 5) + (j >> 5)] >> (j & 31)) & 1u;
            return fmaf(s, SC, ((bias ? bias[(int64_t)q * p.bias_sq + j] : 0.f) + (see ? 0.f : MODCR_NEG)) * LOG2E);
        }
        return bias ? fmaf(s, SC, bias[(int64_t)q * p.bias_sq + j] * LOG2E) : s * SC;
    };
    // DROP: keep / (1 - p) or 0 of key 64 t + lane for query q0 + qi (the wide layout)
    [[maybe_unused]] auto keep = [&](int t, int qi) {
        const int j = t * 64 + lane;
        uint32_t hx, hy;
        attn_drop_words(attn_drop_row(n, p.A, a, q0 + qi, L), j >> 2, p.drop_key, hx, hy);
        return attn_keep_field(hx, hy, j & 3, p.drop_thr16) ? p.drop_keep : 0.f;
    };
    // DALIGN: E of (query q0 + qi, key 64 t + lane), x the keep factor when the map took the dropped probabilities
    [[maybe_unused]] const int T = DALIGN ? p.align_t : 0, R = S - T;
    [[maybe_unused]] const float* galign = DALIGN ? p.d_align + ((int64_t)n * T + q0) * R - T : nullptr;    // row q0 of G, indexed by the key
    [[maybe_unused]] auto ealign = [&](int t, int qi) {
        const int q = q0 + qi, j = t * 64 + lane;
        if (q >= T || j < T || j >= L) return 0.f;
        float e = galign[(uint32_t)qi * (uint32_t)R + (uint32_t)j];
        if constexpr (DROP) {
            if (p.side_post_drop) e *= keep(t, qi);
        }
        return e;
    };
    // ---- sweep 1: statistics --------------------------------------------------------------------------------
    float m[16], lsum[16], o[16];
    [[maybe_unused]] float al[DALIGN ? 16 : 1];     // the align share of D: sum_j e_ij E_ij (keep factor), on the row sum's scale
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) { m[qi] = -INFINITY; lsum[qi] = 0.f; o[qi] = 0.f; }
    if constexpr (DALIGN) {
#pragma unroll
        for (int qi = 0; qi < 16; ++qi) al[qi] = 0.f;
    }
    for (int t = 0; t < ntiles; ++t) {
        load(t);
#pragma unroll
        for (int qi = 0; qi < 16; ++qi) {
            const float s = score(t, qi);
            const float mn = fmaxf(m[qi], wave_max(s));
            const float ms = mn == -INFINITY ? 0.f : mn;
            const float alpha = exp2f(m[qi] - ms);
            const float e = exp2f(s - ms);
            lsum[qi] = lsum[qi] * alpha + wave_sum(e);
            if constexpr (DALIGN) {             // (uniform: the wave holds text rows, the tile region keys)
                if (q0 < T && t * 64 + 63 >= T) al[qi] = al[qi] * alpha + wave_sum(e * ealign(t, qi));
                else al[qi] *= alpha;
            }
            m[qi] = mn;
            if constexpr (DROP) p_img[lane] = e * keep(t, qi);      // the row sum keeps the un-dropped weights
            else p_img[lane] = e;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            float acc = 0.f;
#pragma unroll 8
            for (int j = 0; j < 64; ++j) acc = fmaf(p_img[j], sV[j * 65 + lane], acc);
            o[qi] = o[qi] * alpha + acc;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    // m <- the max the exponentials are taken against, lsum <- 1 / sum, o <- D (formed without hm)
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) {
        const float inv = lsum[qi] > 0.f ? 1.0f / lsum[qi] : 0.f;
        if (m[qi] == -INFINITY) m[qi] = 0.f;
        lsum[qi] = inv;
        o[qi] = wave_sum(o[qi] * d_img[qi * 64 + lane]) * inv;
        if constexpr (DALIGN) o[qi] = fmaf(al[qi], inv, o[qi]);
        if (lane == 0) { stats[q0 + qi] = m[qi]; stats[SP + q0 + qi] = inv; stats[2 * SP + q0 + qi] = o[qi]; }
    }
    // ---- sweep 2: dS, d_bias, dQ ------------------------------------------------------------------------------
    float dq[16];
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) dq[qi] = 0.f;
    for (int t = 0; t < ntiles; ++t) {
        load(t);
#pragma unroll
        for (int qi = 0; qi < 16; ++qi) {
            const float s = score(t, qi);
            const int q = q0 + qi, j = t * 64 + lane;
            float dp = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) dp = fmaf(d_img[qi * 64 + d], sV[lane * 65 + d], dp);
            if constexpr (DROP) dp *= keep(t, qi);
            if constexpr (DALIGN) {
                if (q0 < T && t * 64 + 63 >= T) dp += ealign(t, qi);
            }
            const float ds = exp2f(s - m[qi]) * lsum[qi] * (dp - o[qi]);
            if (dbias && q < S && j < L) dbias[(int64_t)q * L + j] = ds * hm;
            p_img[lane] = ds;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            float acc = 0.f;
#pragma unroll 8
            for (int jj = 0; jj < 64; ++jj) acc = fmaf(p_img[jj], sK[jj * 65 + lane], acc);
            dq[qi] += acc;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    float* dqkv = reinterpret_cast<float*>(p.dqkv) + (int64_t)n * S * 3 * H + a * 64;
#pragma unroll
    for (int qi = 0; qi < 16; ++qi)
        if (q0 + qi < S) dqkv[(int64_t)(q0 + qi) * 3 * H + lane] = dq[qi] * 0.125f * hm;
}

// ---- exact fp32 core, key kernel: 4 waves x 16 keys; Q, dO tiles of 64 queries in LDS -----------------------------------------
template <bool DROP, bool MASK = false, bool DALIGN = false>
__global__ __launch_bounds__(256) void attn_long_bwd_k_f32_kernel(AttnBiasBwdArgs p) {
    extern __shared__ float sm[];
    float* sQ = sm;                          // [64][65]
    float* sD = sQ + 64 * 65;                // [64][65]
    float* sK = sD + 64 * 65;                // per wave [16][64]: the wave's key rows
    float* sV = sK + 4 * 16 * 64;            // per wave [16][64]: their value rows
    float* sW = sV + 4 * 16 * 64;            // per wave [2][64]: p_i, ds_i
    float* sSt = sW + 2 * 4 * 64;            // the tile's max, 1 / sum, D  [3][64]
    const int S = p.S, P = p.P, L = S + P, H = p.H;
    const int n = blockIdx.z, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qtiles = (S + 63) >> 6, SP = qtiles * 64;
    constexpr float SC = 0.125f * LOG2E;
    const float* qkv = reinterpret_cast<const float*>(p.qkv) + (int64_t)n * S * 3 * H + a * 64;
    const float* kvh = reinterpret_cast<const float*>(p.kvh) + (int64_t)n * P * 2 * H + a * 64;
    const float* dctx = reinterpret_cast<const float*>(p.dctx) + (int64_t)n * S * H + a * 64;
    const float* bias = p.bias ? p.bias + (int64_t)n * p.bias_sn + (int64_t)a * p.bias_sa : nullptr;
    const float* stats = p.stats + ((int64_t)n * p.A + a) * 3 * SP;
    const float hm = p.head_mask ? p.head_mask[(int64_t)n * p.head_mask_sn + a] : 1.0f;
    const int k0 = blockIdx.x * 64 + wave * 16;
    [[maybe_unused]] const int T = DALIGN ? p.align_t : 0;
    float* k_img = sK + wave * 16 * 64;
    float* v_img = sV + wave * 16 * 64;
    float* wp = sW + wave * 128;
    float* ws = wp + 64;
    auto krow = [&](int j) { return j < P ? kvh + (int64_t)j * 2 * H : qkv + (int64_t)(j - P) * 3 * H + H; };
#pragma unroll
    for (int kj = 0; kj < 16; ++kj) {        // zeros beyond L
        const int j = k0 + kj;
        k_img[kj * 64 + lane] = j < L ? krow(j)[lane] : 0.f;
        v_img[kj * 64 + lane] = j < L ? krow(j)[H + lane] : 0.f;
    }
    float dk[16], dv[16];
#pragma unroll
    for (int kj = 0; kj < 16; ++kj) { dk[kj] = 0.f; dv[kj] = 0.f; }
    for (int t = 0; t < qtiles; ++t) {
        __syncthreads();
        for (int idx = tid; idx < 64 * 64; idx += 256) {
            const int r = idx >> 6, d = idx & 63, i = t * 64 + r;
            sQ[r * 65 + d] = i < S ? qkv[(int64_t)i * 3 * H + d] : 0.f;
            sD[r * 65 + d] = i < S ? dctx[(int64_t)i * H + d] : 0.f;
        }
        if (tid < 192) sSt[tid] = stats[(tid >> 6) * SP + t * 64 + (tid & 63)];
        __syncthreads();
        const int i = t * 64 + lane;
        const float mi = sSt[lane], ii = sSt[64 + lane], di = sSt[128 + lane];
        // DALIGN: the lane's text row of G, shifted so that the key indexes it (null: a region row, or no text row in this tile)
        [[maybe_unused]] const float* galign = nullptr;
        if constexpr (DALIGN) {
            if (i < T) galign = p.d_align + ((int64_t)n * T + i) * (S - T) - T;
        }
#pragma unroll
        for (int kj = 0; kj < 16; ++kj) {
            const int j = k0 + kj;
            float s = 0.f, dp = 0.f;
#pragma unroll 8
            for (int d = 0; d < 64; ++d) {
                s = fmaf(sQ[lane * 65 + d], k_img[kj * 64 + d], s);
                dp = fmaf(sD[lane * 65 + d], v_img[kj * 64 + d], dp);
            }
            float sv = -INFINITY;
            if constexpr (MASK) {               // 0 / -10000 joins the bias before log2e, as in the forward
                if (j < L) {
                    const int ic = min(i, S - 1);
                    const bool see = (p.bits[((int64_t)n * S + ic) * ((L + 31) >> 5) + (j >> 5)] >> (j & 31)) & 1u;
                    sv = fmaf(s, SC, ((bias ? bias[(int64_t)ic * p.bias_sq + j] : 0.f) + (see ? 0.f : MODCR_NEG)) * LOG2E);
                }
            } else {
                if (j < L) sv = bias ? fmaf(s, SC, bias[(int64_t)min(i, S - 1) * p.bias_sq + j] * LOG2E) : s * SC;
            }
            const float pe = exp2f(sv - mi) * ii;
            if constexpr (DALIGN) {             // + E of (query i, key j), under the keep mask when the map took the dropped probabilities
                const float ea = galign && j >= T && j < L && k0 + 15 >= T ? galign[j] : 0.f;
                float mk = 1.f;
                if constexpr (DROP) {
                    uint32_t hx, hy;
                    attn_drop_words(attn_drop_row(n, p.A, a, i, L), j >> 2, p.drop_key, hx, hy);
                    mk = attn_keep_field(hx, hy, j & 3, p.drop_thr16) ? p.drop_keep : 0.f;
                }
                wp[lane] = pe * mk;
                ws[lane] = pe * ((DROP && p.side_post_drop ? mk * (dp + ea) : fmaf(mk, dp, ea)) - di);
            } else if constexpr (DROP) {        // keep / (1 - p) or 0 of (query i, key j): dV takes the masked probabilities
                uint32_t hx, hy;
                attn_drop_words(attn_drop_row(n, p.A, a, i, L), j >> 2, p.drop_key, hx, hy);
                const float mk = attn_keep_field(hx, hy, j & 3, p.drop_thr16) ? p.drop_keep : 0.f;
                wp[lane] = pe * mk;
                ws[lane] = pe * (mk * dp - di);
            } else {
                wp[lane] = pe;
                ws[lane] = pe * (dp - di);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            float gv = 0.f, gk = 0.f;
#pragma unroll 8
            for (int r = 0; r < 64; ++r) { gv = fmaf(wp[r], sD[r * 65 + lane], gv); gk = fmaf(ws[r], sQ[r * 65 + lane], gk); }
            dv[kj] += gv;
            dk[kj] += gk;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    float* dqkv = reinterpret_cast<float*>(p.dqkv) + (int64_t)n * S * 3 * H + a * 64;
    float* dkvh = reinterpret_cast<float*>(p.dkvh) + (int64_t)n * P * 2 * H + a * 64;
#pragma unroll
    for (int kj = 0; kj < 16; ++kj) {
        const int j = k0 + kj;
        if (j < L) {
            float* ob = j < P ? dkvh + (int64_t)j * 2 * H : dqkv + (int64_t)(j - P) * 3 * H + H;
            ob[lane] = dk[kj] * 0.125f * hm;
            ob[H + lane] = dv[kj] * hm;
        }
    }
}

template <typename K>
int alb_configure(K kernel, int bytes, bool& configured) {
    if (configured) return MODCR_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        modcr_set_error("attn_long_bwd: cannot reserve %d bytes of LDS: %s", bytes, hipGetErrorString(e));
        return MODCR_ERR_LAUNCH;
    }
    configured = true;
    return MODCR_OK;
}

template <bool DROP, bool MASK = false, bool DALIGN = false>
int launch_bf16(const AttnBiasBwdArgs& b, hipStream_t st) {
    const dim3 gq((b.S + 63) / 64, b.A, b.N), gk((b.S + b.P + 63) / 64, b.A, b.N);
    if (!b.bias) hipLaunchKernelGGL((attn_long_bwd_q_kernel<false, false, DROP, MASK, DALIGN>), gq, dim3(ALB::NT), 0, st, b);
    else if (!b.d_bias) hipLaunchKernelGGL((attn_long_bwd_q_kernel<true, false, DROP, MASK, DALIGN>), gq, dim3(ALB::NT), 0, st, b);
    else hipLaunchKernelGGL((attn_long_bwd_q_kernel<true, true, DROP, MASK, DALIGN>), gq, dim3(ALB::NT), 0, st, b);
    int rc = modcr_check_launch("attn_long_bwd_q");
    if (rc != MODCR_OK) return rc;
    if (b.bias) hipLaunchKernelGGL((attn_long_bwd_k_kernel<true, DROP, MASK, DALIGN>), gk, dim3(ALB::NT), 0, st, b);
    else hipLaunchKernelGGL((attn_long_bwd_k_kernel<false, DROP, MASK, DALIGN>), gk, dim3(ALB::NT), 0, st, b);
    return modcr_check_launch("attn_long_bwd_k");
}

template <bool DROP, bool MASK = false, bool DALIGN = false>
int launch_f32(const AttnBiasBwdArgs& b, hipStream_t st) {
    static bool configured_q[MODCR_MAX_DEV] = {}, configured_k[MODCR_MAX_DEV] = {};
    int rc = alb_configure(&attn_long_bwd_q_f32_kernel<DROP, MASK, DALIGN>, ALB::F32_Q, configured_q[modcr_device_index()]);
    if (rc != MODCR_OK) return rc;
    rc = alb_configure(&attn_long_bwd_k_f32_kernel<DROP, MASK, DALIGN>, ALB::F32_K, configured_k[modcr_device_index()]);
    if (rc != MODCR_OK) return rc;
    const dim3 gq((b.S + 63) / 64, b.A, b.N), gk((b.S + b.P + 63) / 64, b.A, b.N);
    hipLaunchKernelGGL((attn_long_bwd_q_f32_kernel<DROP, MASK, DALIGN>), gq, dim3(256), ALB::F32_Q, st, b);
    rc = modcr_check_launch("attn_long_bwd_q_f32");
    if (rc != MODCR_OK) return rc;
    hipLaunchKernelGGL((attn_long_bwd_k_f32_kernel<DROP, MASK, DALIGN>), gk, dim3(256), ALB::F32_K, st, b);
    return modcr_check_launch("attn_long_bwd_k_f32");
}

// the instantiation of a call: DROP from the dropout threshold, MASK / DALIGN from the pointers
template <bool DROP>
int launch_core(const AttnBiasBwdArgs& b, int core, hipStream_t st) {
    const int v = (b.bits ? 1 : 0) | (b.d_align ? 2 : 0);
    if (core == 3) {
        switch (v) {
        case 0: return launch_bf16<DROP>(b, st);
        case 1: return launch_bf16<DROP, true, false>(b, st);
        case 2: return launch_bf16<DROP, false, true>(b, st);
        }
        return launch_bf16<DROP, true, true>(b, st);
    }
    switch (v) {
    case 0: return launch_f32<DROP>(b, st);
    case 1: return launch_f32<DROP, true, false>(b, st);
    case 2: return launch_f32<DROP, false, true>(b, st);
    }
    return launch_f32<DROP, true, true>(b, st);
}

}  // namespace

int modcr_launch_attn_long_bwd(const AttnBiasBwdArgs& b, int core, int32_t dtype, hipStream_t stream) {
    const bool prefix = b.P > 0;
    MODCR_REQUIRE(b.qkv && b.dctx && b.dqkv && b.stats && (b.kvh != nullptr) == prefix && (b.dkvh != nullptr) == prefix &&
                      (b.bias || b.head_mask || b.d_head_mask || b.bits) && (b.bias || !b.d_bias),
                  "attn_long_bwd: null pointer");
    // (the bits and the align map's gradient: no prefix rows, a text block and a region block)
    MODCR_REQUIRE(!(b.bits || b.d_align) || (b.P == 0 && b.S > 256), "attn_long_bwd: mask bits / d_align need P = 0 and S > 256 (S=%d P=%d)", b.S, b.P);
    MODCR_REQUIRE(!b.d_align || (b.align_t > 0 && b.align_t < b.S), "attn_long_bwd: align_t=%d out of range", b.align_t);
    MODCR_REQUIRE((core == 3 || core == 4) && b.N > 0 && b.N <= 65535 && b.A > 0 && b.A <= 65535 && b.H == b.A * 64 && b.S > 0 && b.P >= 0 &&
                      (int64_t)b.S + b.P <= 512,
                  "attn_long_bwd: unsupported call (core=%d S=%d P=%d dropout %s)", core, b.S, b.P, b.drop_thr16 ? "on" : "off");
    // (dropout: the wide counter layout, which exists above 256 keys only and takes (n A + head) 512 x 4 counters in 32 bits)
    MODCR_REQUIRE(b.drop_thr16 == 0 || ((int64_t)b.S + b.P > ATTN_DROP_NARROW_KEYS && (int64_t)b.N * b.A <= ATTN_DROP_WIDE_MAX_NA),
                  "attn_long_bwd: dropout on the streaming cores needs more than 256 keys and N * A = %lld <= 2^21", (long long)b.N * b.A);
    MODCR_REQUIRE(((uintptr_t)b.stats & 15) == 0, "attn_long_bwd: the row statistics are not 16-byte aligned");
    int rc;
    if (core == 3) {
        MODCR_REQUIRE(dtype == MODCR_BF16 && modcr_aligned16(b.qkv) && modcr_aligned16(b.kvh) && modcr_aligned16(b.dctx) && modcr_aligned16(b.dqkv) &&
                          modcr_aligned16(b.dkvh),
                      "attn_long_bwd: the MFMA core takes 16-byte aligned bf16 rows");
        rc = b.drop_thr16 ? launch_core<true>(b, core, stream) : launch_core<false>(b, core, stream);
    } else {
        MODCR_REQUIRE(dtype == MODCR_F32, "attn_long_bwd: the exact core takes fp32 rows and fp32 dctx (bf16 above 256 keys runs the MFMA core)");
        rc = b.drop_thr16 ? launch_core<true>(b, core, stream) : launch_core<false>(b, core, stream);
    }
    if (rc != MODCR_OK || !b.d_head_mask) return rc;
    hipLaunchKernelGGL(attn_long_bwd_dhm_kernel, dim3(b.N * b.A), dim3(64), 0, stream, b.stats, b.d_head_mask, b.S, (b.S + 63) & ~63);
    return modcr_check_launch("attn_long_bwd_dhm");
}
