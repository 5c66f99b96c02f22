// Helpers shared by the attention files -- attn.hip (the forward: tile kernels and host side), attn_long.hip (the streaming forward),
// attn_bwd.hip and attn_bwd_older.hip (the binary-mask backward cores: five-product; older MFMA and exact), attn_bias_bwd.hip and
// attn_long_bwd.hip (the bias family's whole-row and streaming backward cores), attn_bwd_host.hip (the host side of every backward entry; no kernel): the
// attention-probability dropout hash and its host form, LDS row swizzles, the argument blocks, the backward's core ids and launchers.
#pragma once
#include "common.h"

namespace {

// nn.Dropout on the softmax output (modeling_bert.py:69 / v10:101), counter-based, two levels (round 5):
//     base(row, l4)  = fold(cm * 0x85EBCA6B + K),  cm = (row * 4 + l4) * 0x9E3779B1 mod 2^32,  row = (n * A + head) * R + query
//     word(base, j)  = fold(base * C[j] + K),      fold(p) = lo32(p) ^ hi32(p) of the 64-bit sum (one v_mad_u64_u32 + one v_xor)
// R = attn_drop_stride(L) is the row stride of a (sequence, head), chosen per CALL from its key count L = P + S:
//     L <= 256: R = 256, a row has words j = 0..31 -- every kernel of every file, bit for bit what it has always been;
//     L >  256: R = 512, a row has words j = 0..63 -- the wide layout of the streaming cores (attn_long.hip MODE 2, attn_long_bwd.hip DROP).
// With R = 256 the counter of query >= 256 of head a would be the counter of query - 256 of head a + 1; R = 512 keeps the rows of
// 512 queries apart.  The counter row * 4 + l4 is 32 bits wide: the wide layout takes (n * A + head) < 2^21, which the host checks
// (N * A <= 2^21) before it launches.
// K = the 64-bit key derived from (seed, offset) on the host.  Key `key` of a query row takes l4 = (key >> 2) & 3 (its group of
// four inside a 16-key block), word j = 2 * (key >> 4) + ((key >> 1) & 1) and the 16-bit field key & 1 of it (low / high half);
// the weight is kept iff that field, read as a signed 16-bit number, is >= thr16 - 32768 with thr16 = round(p * 2^16) -- one
// saturating packed subtract + arithmetic shift per word gives the 0xffff / 0 keep masks of a packed bf16 pair.
// C[j] = fmix32((j + 1) * 0x9E3779B1) | 1: a compile-time literal wherever j is (the unrolled key tiles of every MFMA kernel).
// The layout does not depend on the token tile, so every kernel (128 / 192 / 256-token tiles, the older kernel, the backward
// cores) regenerates the same mask for P + S <= 256, and the streaming forward and backward cores the same one above.
// Why this form: the round-3/4 hash (Weyl product, two xorshift-multiply rounds per group of four keys, 15-bit fields) was 19 VALU
// instructions per four decisions incl. the compare -- 686 of the ~900 VALU instructions of the forward's phase B, 7 % of the kernel;
// here a lane's base is hashed once per (query, l4) and tile, and every further word costs two instructions: 10 per eight decisions
// + 12 for the compare / mask = 22 against 38.  Statistics (tools/hash_stats.py: keep fraction per field, all 496 field pairs of a
// row's first 16 words, sampled triples, neighbouring l4 / query / head / sequence, cross-seed, histograms; 4 M rows x 3 seeds):
// pair-frequency z-scores rms 1.01, max 3.1 -- noise; a single multiply-fold of the Weyl counter used directly (no second level)
// fails the neighbour tests by 30 sigma, which is why the base is never used as a word.
#define MODCR_DROP_WEYL 0x9E3779B1u
typedef short s16x2_t __attribute__((ext_vector_type(2)));
__host__ __device__ constexpr uint32_t attn_drop_const(int j) {
    uint32_t x = (uint32_t)(j + 1) * 0x9E3779B1u;
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x | 1u;
}
// row stride of a (sequence, head) in the counter: 256 up to 256 keys, 512 above (the wide layout).  Kernels that never see more than
// 256 keys call it with ATTN_DROP_NARROW_KEYS and get the literal.
constexpr int ATTN_DROP_NARROW_KEYS = 256;
constexpr int ATTN_DROP_WIDE_KEYS = 512;
constexpr int64_t ATTN_DROP_WIDE_MAX_NA = 1ll << 21;        // N * A of a wide call: (N A) 512 x 4 counters fit 32 bits
__host__ __device__ constexpr int attn_drop_stride(int L) { return L > ATTN_DROP_NARROW_KEYS ? ATTN_DROP_WIDE_KEYS : ATTN_DROP_NARROW_KEYS; }
// the counter row of (sequence n, head, query) in a call of A heads and L keys
__host__ __device__ constexpr uint32_t attn_drop_row(int n, int A, int head, int query, int L) {
    return (uint32_t)((n * A + head) * attn_drop_stride(L) + query);
}
__device__ __forceinline__ uint32_t attn_drop_fold(uint32_t a, uint32_t c, uint64_t k) {
    const uint64_t p = (uint64_t)a * c + k;
    return (uint32_t)p ^ (uint32_t)(p >> 32);
}
// row = attn_drop_row(n, A, head, query, L) (tile row: prefix rows count), l4 = 0..3
__device__ __forceinline__ uint32_t attn_drop_base(uint32_t row, uint32_t l4, uint64_t k) {
    return attn_drop_fold((row * 4u + l4) * MODCR_DROP_WEYL, 0x85EBCA6Bu, k);
}
__device__ __forceinline__ uint32_t attn_drop_word(uint32_t base, int j, uint64_t k) { return attn_drop_fold(base, attn_drop_const(j), k); }
// 0xffff in each 16-bit half of w that is kept; thrm1_2 = ((thr16 - 32769) & 0xffff) * 0x00010001
__device__ __forceinline__ uint32_t attn_keep2(uint32_t w, uint32_t thrm1_2) {
    s16x2_t d = __builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2_t, thrm1_2), __builtin_bit_cast(s16x2_t, w));   // < 0 iff field >= thr
    d = d >> 15;
    return __builtin_bit_cast(uint32_t, d);
}
__host__ __device__ inline uint32_t attn_thr16(float p) {
    uint32_t t = (uint32_t)((double)p * 65536.0 + 0.5);
    return t < 1u ? 1u : (t > 65535u ? 65535u : t);
}
__host__ __device__ inline uint32_t attn_thrm1_2(uint32_t thr16) { return ((thr16 - 32769u) & 0xffffu) * 0x00010001u; }
// the two words of the 4-key group `g4` = key >> 2 (0..63) of a row: x decides keys 4 g4, 4 g4 + 1, y keys 4 g4 + 2, 4 g4 + 3
__device__ __forceinline__ void attn_drop_words(uint32_t row, int g4, uint64_t k, uint32_t& x, uint32_t& y) {
    const uint32_t b = attn_drop_base(row, (uint32_t)(g4 & 3), k);
    x = attn_drop_word(b, (g4 >> 2) * 2, k);
    y = attn_drop_word(b, (g4 >> 2) * 2 + 1, k);
}
// the keep decision of key (4 g4 + f), f = 0..3, from the words of its group
__device__ __forceinline__ bool attn_keep_field(uint32_t x, uint32_t y, int f, uint32_t thr16) {
    const uint32_t w = (f & 2) ? y : x;
    return (int)(short)(w >> ((f & 1) * 16)) >= (int)thr16 - 32768;
}
// value of lane (quad base + E) in every lane of the quad (DPP quad_perm broadcast)
template <int E> __device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, E * 0x55, 0xf, 0xf, true);
}
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
// the eight weights of a lane in one 32-key tile kt (keys 32 kt + 16 kb + 4 l4 + e: pb[4 kb + e]); base = attn_drop_base(row, l4)
// (the multipliers are made opaque SGPR values: left visible, the compiler chains the words as P[j+1] = P[j] + base * (C[j+1] - C[j]) --
// a serial v_mad_u64_u32 chain plus a v_sub correction of the high word whenever the difference wraps)
template <int KT> __device__ __forceinline__ bf16x8 attn_drop8(bf16x8 pb, uint32_t base, uint64_t k, uint32_t thrm1_2) {
    u32x4_t w = __builtin_bit_cast(u32x4_t, pb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {                           // i = 2 kb + (e >> 1)
        uint32_t c = attn_drop_const(4 * KT + i);
        asm volatile("" : "+s"(c));
        w[i] &= attn_keep2(attn_drop_fold(base, c, k), thrm1_2);
    }
    return __builtin_bit_cast(bf16x8, w);
}
// the same with a run-time tile index (the exact pass)
__device__ __forceinline__ bf16x8 attn_drop8_rt(bf16x8 pb, uint32_t base, int kt, uint64_t k, uint32_t thrm1_2) {
    u32x4_t w = __builtin_bit_cast(u32x4_t, pb);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] &= attn_keep2(attn_drop_word(base, 4 * kt + i, k), thrm1_2);
    return __builtin_bit_cast(bf16x8, w);
}

__device__ __forceinline__ int swz128(int row, int chunk) { return (row << 7) + (((chunk ^ (row >> 1)) & 7) << 4); }
__device__ __forceinline__ int swz64(int row, int chunk) { return (row << 6) + (((chunk ^ (row >> 2)) & 3) << 4); }

typedef __attribute__((address_space(3))) bf16x4* lds_tr_b;

// Transposed fragment of a swz128 row image (attn_bias_bwd.hip, attn_long_bwd.hip; as attn_bwd_mfma_kernel's): feature
// 16 db + l15, tokens tok0 + 4 l4 + {0..3} and tok0 + 16 + 4 l4 + {0..3}.  The gather crosses lanes: call it with every lane of
// the wave active.
__device__ __forceinline__ bf16x8 abb_tr8(const unsigned char* img, int tok0, int db, int l15, int l4) {
    const int r = tok0 + 4 * l4 + (l15 >> 2);
    const int ch = db * 2 + ((l15 & 3) >> 1), within = (l15 & 1) * 8;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_b)(img + swz128(r, ch) + within));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr_b)(img + swz128(r + 16, ch) + within));
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
    return o;
}

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr float LOG2E = 1.44269504088896340736f;

// attention-probability dropout as the host hands it to a kernel: the 64-bit key of (seed, offset), thr16 = round(p * 2^16) (0 = off)
// and 1 / (1 - p); thr2 = the packed threshold of the bf16 tile kernels
struct AttnDrop {
    uint64_t key; uint32_t thr16; float keep;
    uint32_t thr2() const { return thr16 ? attn_thrm1_2(thr16) : 0; }
};
inline AttnDrop attn_drop(float attn_p, uint64_t seed, uint64_t offset) {
    if (!(attn_p > 0.f)) return {0, 0, 1.f};
    return {seed + offset * 0x9E3779B97F4A7C15ull, attn_thr16(attn_p), 1.0f / (1.0f - attn_p)};
}

// token tile of attn_bwd_mfma_kernel (AB::LP) and key limit of the bf16 MFMA backward cores: what the backward's route function compares with
constexpr int ATTN_BWD_MFMA_LP = 192;

}  // namespace

// The cores of the attention backward, as attn_bwd_route() (attn_bwd_host.hip) names them.  Mask family (key_mask / dense bits):
// FIVE = attn_bwd5_kernel / attn_bwd6_kernel, MFMA / MFMA_DALIGN = attn_bwd_mfma_kernel<bf16, DALIGN>, EXACT = attn_bwd_f32_kernel;
// bias family (additive bias, head mask, prefix rows): BIAS_MFMA / BIAS_EXACT = the whole-row cores of attn_bias_bwd.hip, STREAM /
// STREAM_EXACT = the streaming cores of attn_long_bwd.hip above 256 keys.
enum AttnBwdCore {
    ATTN_BWD_REFUSED = 0, ATTN_BWD_FIVE, ATTN_BWD_MFMA, ATTN_BWD_MFMA_DALIGN, ATTN_BWD_EXACT,
    ATTN_BWD_BIAS_MFMA, ATTN_BWD_BIAS_EXACT, ATTN_BWD_STREAM, ATTN_BWD_STREAM_EXACT
};

struct AttnBwdArgs {
    const float* qkv; const void* dctx; const float* key_mask; const uint32_t* bits; float* dqkv;
    const bf16* qkvb;               // MFMA kernel: the recomputed q | k | v rows as bf16 (what the forward's images hold), qkv unused
    int out_bf16;                   // MFMA kernel: dq | dk | dv rows leave as bf16 (the operand dtype of the GEMMs that consume them)
    // attention-probability dropout of the forward: 0 = off, else thr16 = round(p * 2^16); the 64-bit key; 1 / (1 - p)
    uint32_t drop_thr16;
    uint64_t drop_key;
    float drop_keep;
    int side_post_drop;             // MODCR_ATTN_SIDE_POST_DROPOUT: d_align belongs to a map of the probabilities after the dropout
    // gradient of the head-summed text -> region map (align map of modcr_qkv_attn_fwd) [N, T, R], or NULL: added to dP of
    // every head for query < T, key >= T (un-dropped probabilities; with side_post_drop under the forward's dropout mask)
    const float* d_align;
    int align_t;
    // five-product core (attn_bwd.hip): the forward's context rows [N, S, H] (delta = rowsum(dO o O)) and its log2-domain
    // row statistics lse[N, A, S] = log2(sum_j exp2(score_ij log2e)) (modcr_qkv_attn_lse_fwd); NULL = the older cores recompute them
    const bf16* ctx;
    const float* lse;
    // Q | K | V images the forward dumped (modcr_qkv_attn_lse_fwd's qkv_dump: [N][A][3][LP][64], Q scaled and chunk-averaged), or NULL
    const bf16* dump;
    // with dump + d_align: delta_align[N, A, S] = sum_j P_ij d_align_ij (text query i, region keys j), written by attn_dalign_delta_kernel
    float* delta_align;
    int N, S, H, A;
    int debug;      // tuning build only (MODCR_ATTN_BWD_DEBUG): 1 = return once the first images are built, 2 = no sub-pass Q, 4 = no sub-pass K
};

// attn_bwd.hip: launches attn_bwd5_kernel on `b` (bf16 rows, 0 < S <= 192, lse and ctx given, no align-map gradient)
__attribute__((visibility("hidden"))) int modcr_launch_attn_bwd5(const AttnBwdArgs& b, hipStream_t stream);
// attn_bwd_older.hip: launches the older cores on `b`: ATTN_BWD_MFMA / ATTN_BWD_MFMA_DALIGN (bf16 rows in and out, S <= 192) or ATTN_BWD_EXACT
// (fp32 rows in and out, S <= 256; dctx in `dtype`)
__attribute__((visibility("hidden"))) int modcr_launch_attn_bwd_older(const AttnBwdArgs& b, AttnBwdCore core, int32_t dtype, hipStream_t stream);

// attn_bias_bwd.hip: the attention core backward under an additive bias and / or a head mask, S queries against L = P + S keys
// (modcr_qkv_attn_bias_bwd: P = 0; modcr_qkv_attn_prefix_bwd: P > 0 prefix keys).  The own rows' q | k | v projection qkv [N*S][3H]
// and, with P > 0, the prefix rows' k | v projection kvh [N*P][2H] come in; dq | dk | dv of the own rows (dqkv, same layout) and
// dk | dv of the prefix rows (dkvh, same layout) go out; d_bias = dS [N, A, S, L] fp32 when wanted.
struct AttnBiasBwdArgs {
    const void* qkv; const void* kvh; const void* dctx;    // core 1: bf16 rows in and out; core 2: fp32 rows, dctx in the storage dtype
    void* dqkv; void* dkvh;                                 // kvh, dkvh: NULL exactly when P == 0
    // bias[n sn + a sa + q sq + j] fp32, j over the L keys (strides in elements, 0 = broadcast; NULL = no bias), head_mask[n hsn + a]
    // (NULL = 1)
    const float* bias; int64_t bias_sn, bias_sa, bias_sq;
    const float* head_mask; int64_t head_mask_sn;
    float* d_bias;                                          // or NULL
    // the forward's attention-probability dropout: 0 = off, else thr16 = round(p * 2^16); the 64-bit key; 1 / (1 - p)
    uint32_t drop_thr16;
    uint64_t drop_key;
    float drop_keep;
    int N, S, P, H, A;
    // fp32 [N, A] or NULL: the gradient of the head's multiplier, d_hm[n, a] = sum_i dctx_i . (P'.V)_i (the DHM instantiations; one
    // lane writes each element).  head_mask == NULL then stands for a mask of ones.  Last, so that every other field keeps its offset.
    float* d_head_mask;
    // attn_long_bwd.hip only: the per-row statistics fp32 [N A][3][SP] (row max, 1 / row sum, D; SP = S rounded up to 64), 16-byte
    // aligned, written by its query kernel and read by its key kernel.  The whole-row cores never look at it.
    float* stats;
    // modcr_qkv_attn_long_align_bwd, attn_long_bwd.hip only (P = 0, S > 256); at the end, so that every other field keeps its offset.
    // bits: u32 [N, S, ceil(S / 32)] dense mask, bit j of row (n, i) clear = -10000 on top of the bias (the MASK instantiations), or
    // NULL.  d_align: fp32 [N, T, R] gradient of the head-summed text -> region map, T = align_t, R = S - T (the DALIGN
    // instantiations), or NULL: E_ij = d_align[n, i, j - T] for i < T <= j joins dP of every head -- under the keep mask with
    // side_post_drop (the map summed the probabilities after the dropout), plainly without.
    const uint32_t* bits;
    const float* d_align;
    int align_t;
    int side_post_drop;
};
// core: 1 = attn_bias_bwd_mfma_kernel (bf16, P + S <= 192), 2 = attn_bias_bwd_f32_kernel (P + S <= 256); prefix rows where b.P > 0
__attribute__((visibility("hidden"))) int modcr_launch_attn_bias_bwd(const AttnBiasBwdArgs& b, int core, int32_t dtype, hipStream_t stream);
// attn_long_bwd.hip: the streaming cores for 256 < P + S <= 512 keys (dropout: the wide counter layout); core: 3 = the bf16 MFMA kernels, 4 = the exact fp32 kernels
// (fp32 dtype only: its dctx is fp32); b.stats given
__attribute__((visibility("hidden"))) int modcr_launch_attn_long_bwd(const AttnBiasBwdArgs& b, int core, int32_t dtype, hipStream_t stream);

// attn_long.hip: the streaming attention core (P + S <= 512) over q | k | v rows the dispatcher projected: qx [N*S][3H] (queries,
// chunk-mean applied), qh [N*P][3H] (prefix rows) -- bf16 or fp32 as `dtype`.  Binary masks (key_mask / bits: above 256 keys, no
// dropout), or -- bias and / or head_mask set -- the additive-bias variant of modcr_qkv_attn_bias_fwd at any P + S <= 512.
struct AttnLongArgs {
    const void* qx; const void* qh;
    const float* key_mask; const uint32_t* bits;
    void* ctx; float* probs; float* align_map;
    int N, S, P, H, A, align_t;
    // bias variant: bias[n sn + a sa + q sq + j] fp32 (strides in elements, 0 = broadcast; NULL = no bias), head_mask[n hsn + a]
    // (NULL = 1); dropout of the probabilities (counter stride attn_drop_stride(P + S)): 0 = off, else thr16 = round(p * 2^16), the 64-bit key, 1 / (1 - p)
    const float* bias; int64_t bias_sn, bias_sa, bias_sq;
    const float* head_mask; int64_t head_mask_sn;
    uint32_t drop_thr16;
    uint64_t drop_key;
    float drop_keep;
    int side_post_drop;
    // modcr_qkv_attn_long_align_fwd: bits (no prefix rows, P + S > 256) is read by the BIAS variant, 0 / -10000 on top of the bias; with
    // it the bits alone select that variant.  0: the bias variant never looks at bits.  Last, so that every other field keeps its offset.
    int bits_on_bias;
};
// ev0 / ev1 (or NULL): stamped at the start and the end of the kernel (modcr_time_next_attn)
__attribute__((visibility("hidden"))) int modcr_launch_attn_long(const AttnLongArgs& p, int32_t dtype, hipStream_t stream, hipEvent_t ev0,
                                                                 hipEvent_t ev1);
