// Host side of the attention backward (CDNA4 / gfx950): the ten entries modcr_qkv_attn_bwd, _dropout_bwd, _lse_bwd, _opt_bwd (the mask
// family: key_mask / dense bits, S <= 256, no prefix rows) and _bias_bwd, _prefix_bwd, _gate_bwd, _long_bwd, _long_drop_bwd (the bias
// family: additive bias and / or head mask, P >= 0 prefix rows, P + S <= 256, or <= 512 from _long_bwd -- without attention dropout
// above 256 keys --, _long_drop_bwd -- with it, the wide counter layout -- and _long_align_bwd -- with dense mask bits and the align
// map's gradient on top, above 256 keys, no prefix rows), their _workspace and _route companions.
// No kernel lives here: the cores are in attn_bwd.hip (five-product), attn_bwd_older.hip (older MFMA, exact), attn_bias_bwd.hip (bias MFMA, bias exact) and
// attn_long_bwd.hip (stream, stream exact), behind the four launchers of attn_common.h.
//
// Every entry fills an AttnBwdCall, states what only it requires, and calls attn_bwd(): one check function per family, one route
// function, one workspace layout, one step sequence --
//     1. recompute the own rows' q | k | v (unless the forward dumped its images), chunk-mean queries as the forward
//     2. the prefix rows' k | v
//     3. the core: dq | dk | dv of the own rows, dk | dv of the prefix rows
//     4. the chunk mean is its own adjoint: dq rows of a chunk <- their mean (v10:66-78)
//     5. own rows:    dX = dqkv . Wqkv (+ dx_residual);  dWqkv (+)= dqkv^T . X;  dbqkv (+)= column sums
//     6. prefix rows: d_hist = d(k|v) . Wqkv[H:3H];  dWqkv[H:3H] += d(k|v)^T . hist;  dbqkv[H:3H] += column sums (rows H..3H of wqkv /
//        bqkv are a contiguous [2H, H] sub-block, ldw = H)
#include "common.h"
#include "attn_common.h"

namespace {

// One backward call: the operands of all eight entries by name.  A null pointer or a zero means "not given".
struct AttnBwdCall {
    const char* who;                // the entry's name in the bias family's messages (the mask family's all say qkv_attn_bwd)
    bool bias_family;
    int max_keys;                   // bias family: 256, or 512 from modcr_qkv_attn_long_bwd / _long_drop_bwd
    bool wide_dropout;              // bias family: attention dropout above 256 keys is served (modcr_qkv_attn_long_drop_bwd: the wide counter layout)
    const void* dctx; const void* x; const void* hist; const void* wqkv; const float* bqkv;
    const float* key_mask; const uint32_t* bits;                                            // mask family
    const float* bias; int64_t bias_sn, bias_sa, bias_sq; const float* head_mask; int64_t head_mask_sn;    // bias family
    const int32_t* chunk_id; int32_t chunk_t;
    const float* dx_residual; void* dx; void* d_hist; float* dwqkv; float* dbqkv; int32_t accumulate;
    float* d_bias; float* d_head_mask;                                                      // bias family
    int32_t N, S, P, H, A;
    float attn_p; uint64_t seed, offset;
    // mask family.  ctx + lse (both or neither; bf16): the forward's context rows and the row statistics modcr_qkv_attn_lse_fwd wrote:
    // with them the core is the five-product kernel (P rebuilt from lse, delta = rowsum(dO o O)); without them, or with an align-map
    // gradient and no dump, the older core recomputes the statistics (eight products).  flags: MODCR_ATTN_SIDE_POST_DROPOUT = d_align is
    // the gradient of an align map that summed the probabilities AFTER the dropout (modcr_qkv_attn_opt_fwd with the same flag): it enters
    // dP under the forward's mask, m / (1 - p) o d_align
    const float* d_align; int32_t align_t; const void* ctx; const float* lse; const void* dump; int32_t flags;
    void* workspace; int64_t workspace_bytes; int32_t dtype; modcr_stream_t stream;
};

// The workspace: q | k | v and dq | dk | dv rows of the own rows (rows_x each), k | v and dk | dv rows of the prefix rows (rows_h
// each; 0 without), then the GEMMs' sub-workspace (the larger of the two sets' needs) and, above 256 keys only (the streaming cores),
// their per-row statistics fp32 [N A][3][S rounded up to 64] at the end
struct AttnBwdWs {
    int64_t rows_x, rows_h, sub, stats;
    int64_t bytes() const { return 2 * rows_x + 2 * rows_h + sub + stats; }
};
int64_t attn_bwd_sub_ws(int32_t M, int32_t K3, int32_t H) {
    const int64_t a = modcr_linear_bwd_input_workspace(M, K3, H), b = modcr_linear_bwd_weight_workspace(M, K3, H);
    return ((a > b ? a : b) + 255) & ~(int64_t)255;
}
AttnBwdWs attn_bwd_ws(int32_t N, int32_t S, int32_t P, int32_t H, int max_keys = 256) {
    AttnBwdWs w;
    w.stats = (int64_t)P + S <= 256 || max_keys <= 256 ? 0 : (((int64_t)N * (H / 64) * 3 * ((S + 63) & ~63) * (int64_t)sizeof(float)) + 255) & ~(int64_t)255;
    w.rows_x = (((int64_t)N * S * 3 * H * (int64_t)sizeof(float)) + 255) & ~(int64_t)255;
    w.rows_h = (((int64_t)N * P * 2 * H * (int64_t)sizeof(float)) + 255) & ~(int64_t)255;
    w.sub = attn_bwd_sub_ws(N * S, 3 * H, H);
    if (P > 0) {
        const int64_t h = attn_bwd_sub_ws(N * P, 2 * H, H);
        if (h > w.sub) w.sub = h;
    }
    return w;
}

// The core of a call: the one place the choice is made, and the only reader of MODCR_ATTN_BWD_VALU and MODCR_ATTN_BWD_OLD (tuning
// build only, common.h).  Looks at the family, the shape, dtype and max_keys, and in the mask family at lse, d_align and dump.  A call is
// routed by its family's check function once its shape is known good; the bias family's shape is looked at here too (ATTN_BWD_REFUSED), for
// its _route entries.
AttnBwdCore attn_bwd_route(const AttnBwdCall& c) {
    const bool bf = c.dtype == MODCR_BF16;
    if (!c.bias_family) {
        if (!(bf && c.S <= ATTN_BWD_MFMA_LP && !modcr_knob_set("MODCR_ATTN_BWD_VALU"))) return ATTN_BWD_EXACT;
        if (c.lse && (!c.d_align || c.dump) && !modcr_knob_set("MODCR_ATTN_BWD_OLD")) return ATTN_BWD_FIVE;
        return c.d_align ? ATTN_BWD_MFMA_DALIGN : ATTN_BWD_MFMA;
    }
    if (c.N <= 0 || c.S <= 0 || c.P < 0 || (int64_t)c.P + c.S > c.max_keys || c.A <= 0 || c.H != c.A * 64 || (!bf && c.dtype != MODCR_F32))
        return ATTN_BWD_REFUSED;
    if (c.P + c.S > 256) return bf ? ATTN_BWD_STREAM : ATTN_BWD_STREAM_EXACT;
    return bf && c.P + c.S <= ATTN_BWD_MFMA_LP ? ATTN_BWD_BIAS_MFMA : ATTN_BWD_BIAS_EXACT;
}
// what the bias family's _route entries answer and its launchers take: 0 = refused, 1 = MFMA core, 2 = exact core, 3 = stream, 4 = stream exact
int attn_bwd_core_number(AttnBwdCore core) { return core >= ATTN_BWD_BIAS_MFMA ? core - ATTN_BWD_BIAS_MFMA + 1 : 0; }
int attn_bias_bwd_route(int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, int32_t dtype, int max_keys) {
    AttnBwdCall c = {};
    c.bias_family = true; c.max_keys = max_keys; c.N = N; c.S = S; c.P = P; c.H = H; c.A = A; c.dtype = dtype;
    return attn_bwd_core_number(attn_bwd_route(c));
}
// dtype of the q | k | v and dq | dk | dv rows: bf16 at the MFMA cores (what the forward's LDS images held; half the bytes), fp32 at the
// exact cores, whatever the storage dtype
int32_t attn_bwd_rows_dtype(AttnBwdCore core) {
    return core == ATTN_BWD_EXACT || core == ATTN_BWD_BIAS_EXACT || core == ATTN_BWD_STREAM_EXACT ? MODCR_F32 : MODCR_BF16;
}

// What the mask family refuses (no 16-byte and no workspace alignment check here: the five-product launcher has its own).  The workspace
// layout and the route are worked out where the checks first need them, on a validated shape: ws and core are theirs on MODCR_OK.
int attn_bwd_mask_checks(const AttnBwdCall& c, AttnBwdWs& ws, AttnBwdCore& core) {
    MODCR_REQUIRE(c.dctx && c.x && c.wqkv && c.bqkv && c.dx && c.dwqkv && c.dbqkv, "qkv_attn_bwd: null pointer");
    MODCR_REQUIRE((c.flags & ~MODCR_ATTN_SIDE_POST_DROPOUT) == 0, "qkv_attn_bwd: unknown flags 0x%x", c.flags);
    MODCR_REQUIRE(!c.d_align || (c.align_t > 0 && c.align_t < c.S), "qkv_attn_bwd: align_t=%d out of range", c.align_t);
    MODCR_REQUIRE((c.ctx == nullptr) == (c.lse == nullptr), "qkv_attn_bwd: ctx and lse come together");
    MODCR_REQUIRE(!c.dump || (c.lse && c.dtype == MODCR_BF16 && c.S > 64 && c.S <= 192),
                  "qkv_attn_bwd: the forward's q|k|v dump is used with ctx + lse, bf16, 64 < S <= 192");
    MODCR_REQUIRE(c.attn_p >= 0.f && c.attn_p < 1.f, "qkv_attn_bwd: attention dropout p=%g out of [0, 1)", c.attn_p);
    // (every core regenerates the forward's mask from (seed, offset): the MFMA cores at S <= 192, the exact core elsewhere and in fp32)
    MODCR_REQUIRE(c.attn_p == 0.f || c.S <= 256, "qkv_attn_bwd: attention-probability dropout needs S <= 256 (S=%d)", c.S);
    MODCR_REQUIRE(c.N > 0 && c.S > 0 && c.S <= 256 && c.A > 0 && c.H == c.A * 64, "qkv_attn_bwd: bad shape (N=%d S=%d H=%d A=%d)", c.N, c.S, c.H, c.A);
    MODCR_REQUIRE(c.key_mask || c.bits, "qkv_attn_bwd: need key_mask or dense_mask_bits");
    MODCR_REQUIRE(c.dtype == MODCR_BF16 || c.dtype == MODCR_F32, "qkv_attn_bwd: unknown dtype %d", c.dtype);
    ws = attn_bwd_ws(c.N, c.S, 0, c.H);
    MODCR_REQUIRE(c.workspace && c.workspace_bytes >= ws.bytes(), "qkv_attn_bwd: workspace %lld < %lld bytes", (long long)c.workspace_bytes,
                  (long long)ws.bytes());
    core = attn_bwd_route(c);
    return MODCR_OK;
}

// What the bias family refuses (no flags, ctx / lse or dump here: its entries have none)
int attn_bwd_bias_checks(const AttnBwdCall& c, AttnBwdWs& ws, AttnBwdCore& core) {
    const char* who = c.who;
    const int32_t N = c.N, S = c.S, P = c.P, H = c.H, A = c.A;
    MODCR_REQUIRE(c.dctx && c.x && c.wqkv && c.bqkv && c.dx && (c.d_hist || !P) && c.dwqkv && c.dbqkv, "%s: null pointer", who);
    MODCR_REQUIRE(c.dtype == MODCR_BF16 || c.dtype == MODCR_F32, "%s: unknown dtype %d", who, c.dtype);
    MODCR_REQUIRE(N > 0 && S > 0 && A > 0, "%s: bad shape (N=%d S=%d P=%d H=%d A=%d)", who, N, S, P, H, A);
    MODCR_REQUIRE(H == A * 64, "%s: head size must be 64 (H=%d, A=%d)", who, H, A);
    if ((int64_t)P + S > c.max_keys) {
        modcr_set_error("%s: P + S = %lld keys (P=%d) exceeds the %d-key limit of the attention backward", who, (long long)P + S, P, c.max_keys);
        return MODCR_ERR_UNSUPPORTED;
    }
    if ((int64_t)P + S > 256 && c.attn_p > 0.f && !c.wide_dropout) {
        modcr_set_error("%s: attention-probability dropout (p=%g) is not implemented above 256 keys (P+S=%d)", who, c.attn_p, P + S);
        return MODCR_ERR_UNSUPPORTED;
    }
    // (the wide counter layout: (n A + head) x 512 rows x 4 counters in 32 bits)
    MODCR_REQUIRE(!((int64_t)P + S > 256 && c.attn_p > 0.f) || (int64_t)N * A <= ATTN_DROP_WIDE_MAX_NA,
                  "%s: N * A = %lld (N=%d, A=%d) exceeds the 2^21 (sequence, head) pairs of the wide dropout counter", who, (long long)N * A, N, A);
    // (with d_head_mask a missing head_mask is a mask of ones: the head-importance call)
    MODCR_REQUIRE(c.bias || c.head_mask || c.d_head_mask || c.bits, "%s: neither bias nor head_mask%s", who,
                  P ? "" : " (that call belongs to modcr_qkv_attn_opt_bwd)");
    MODCR_REQUIRE(c.bias || !c.d_bias, "%s: d_bias without a bias", who);
    MODCR_REQUIRE(c.attn_p >= 0.f && c.attn_p < 1.f, "%s: attention dropout p=%g out of [0, 1)", who, c.attn_p);
    MODCR_REQUIRE(c.bias_sn >= 0 && c.bias_sa >= 0 && c.bias_sq >= 0 && c.head_mask_sn >= 0, "%s: negative stride", who);
    // (the cores address a (sequence, head) slice of the bias with 32-bit element offsets)
    MODCR_REQUIRE(c.bias_sq <= (1 << 20), "%s: bias query stride %lld exceeds 2^20 elements", who, (long long)c.bias_sq);
    MODCR_REQUIRE(((uintptr_t)c.bias & 3) == 0 && ((uintptr_t)c.head_mask & 3) == 0 && ((uintptr_t)c.d_bias & 3) == 0 &&
                      ((uintptr_t)c.d_head_mask & 3) == 0,
                  "%s: bias / head_mask / d_bias%s not 4-byte aligned", who, c.d_head_mask ? " / d_head_mask" : "");
    MODCR_REQUIRE(!c.chunk_id || (c.chunk_t > 0 && c.chunk_t <= S), "%s: chunk_t=%d out of range", who, c.chunk_t);
    MODCR_REQUIRE(c.dtype != MODCR_BF16 || (modcr_aligned16(c.dctx) && modcr_aligned16(c.x) && modcr_aligned16(c.hist) && modcr_aligned16(c.wqkv) &&
                                            modcr_aligned16(c.dx) && modcr_aligned16(c.d_hist)),
                  "%s(bf16): 16-byte alignment", who);
    ws = attn_bwd_ws(N, S, P, H, c.max_keys);
    MODCR_REQUIRE(c.workspace && c.workspace_bytes >= ws.bytes() && modcr_aligned16(c.workspace), "%s: workspace %lld < %lld bytes (or unaligned)", who,
                  (long long)c.workspace_bytes, (long long)ws.bytes());
    core = attn_bwd_route(c);
    // (the streaming kernels' grid is (block, head, sequence))
    MODCR_REQUIRE((core != ATTN_BWD_STREAM && core != ATTN_BWD_STREAM_EXACT) || (N <= 65535 && A <= 65535),
                  "%s: grid of N=%d sequences x A=%d heads too large", who, N, A);
    return MODCR_OK;
}

// what the gate entry and modcr_qkv_attn_long_bwd check before the shared body: P >= 0, hist / d_hist exactly with prefix rows, no
// chunk mean with them
int attn_gate_precheck(const AttnBwdCall& c) {
    MODCR_REQUIRE(c.P >= 0, "%s: bad shape (P=%d)", c.who, c.P);
    MODCR_REQUIRE((c.hist != nullptr) == (c.P > 0) && (c.d_hist != nullptr) == (c.P > 0),
                  "%s: hist and d_hist are given exactly with prefix rows (P=%d, hist %s, d_hist %s)", c.who, c.P, c.hist ? "given" : "null",
                  c.d_hist ? "given" : "null");
    MODCR_REQUIRE(!c.chunk_id || c.P == 0, "%s: no chunk-mean queries with prefix rows (P=%d)", c.who, c.P);
    return MODCR_OK;
}

// the argument block of the mask family's cores (qkv / dqkv: the row areas of the workspace)
AttnBwdArgs attn_bwd_mask_args(const AttnBwdCall& c, AttnBwdCore core, float* qkv, float* dqkv) {
    AttnBwdArgs b;
    b.qkv = qkv; b.qkvb = reinterpret_cast<const bf16*>(qkv); b.dctx = c.dctx; b.key_mask = c.key_mask; b.bits = c.bits; b.dqkv = dqkv;
    b.N = c.N; b.S = c.S; b.H = c.H; b.A = c.A; b.out_bf16 = core != ATTN_BWD_EXACT;
    const AttnDrop d = attn_drop(c.attn_p, c.seed, c.offset);     // (as the forward)
    b.drop_thr16 = d.thr16; b.drop_key = d.key; b.drop_keep = d.keep;
    b.side_post_drop = (c.attn_p > 0.f && (c.flags & MODCR_ATTN_SIDE_POST_DROPOUT)) ? 1 : 0;
    b.d_align = c.d_align; b.align_t = c.align_t;
    b.ctx = reinterpret_cast<const bf16*>(c.ctx); b.lse = c.lse; b.dump = reinterpret_cast<const bf16*>(c.dump);
    b.delta_align = c.dump ? qkv : nullptr;                 // (with the dump the q|k|v area of the workspace is free: N A S floats of it)
    b.debug = modcr_knob_int("MODCR_ATTN_BWD_DEBUG", 0);    // tuning build only
    return b;
}

// ... and of the bias family's (kvh / dkvh: null without prefix rows; stats: the streaming cores' statistics area, else null)
AttnBiasBwdArgs attn_bwd_bias_args(const AttnBwdCall& c, void* qkv, void* dqkv, void* kvh, void* dkvh, float* stats) {
    AttnBiasBwdArgs b;
    b.qkv = qkv; b.kvh = kvh; b.dctx = c.dctx; b.dqkv = dqkv; b.dkvh = dkvh;
    b.bias = c.bias; b.bias_sn = c.bias_sn; b.bias_sa = c.bias_sa; b.bias_sq = c.bias_sq;
    b.head_mask = c.head_mask; b.head_mask_sn = c.head_mask_sn;
    b.d_bias = c.d_bias; b.d_head_mask = c.d_head_mask;
    const AttnDrop d = attn_drop(c.attn_p, c.seed, c.offset);     // (as the forward)
    b.drop_thr16 = d.thr16; b.drop_key = d.key; b.drop_keep = d.keep;
    b.N = c.N; b.S = c.S; b.P = c.P; b.H = c.H; b.A = c.A;
    b.stats = stats;
    // (modcr_qkv_attn_long_align_bwd only: every other bias-family entry leaves them null / 0)
    b.bits = c.bits; b.d_align = c.d_align; b.align_t = c.align_t;
    b.side_post_drop = (c.attn_p > 0.f && (c.flags & MODCR_ATTN_SIDE_POST_DROPOUT)) ? 1 : 0;
    return b;
}

// Every backward entry.
int attn_bwd(const AttnBwdCall& c) {
    const int32_t N = c.N, S = c.S, P = c.P, H = c.H, dtype = c.dtype;
    AttnBwdWs ws;
    AttnBwdCore core;
    int rc = c.bias_family ? attn_bwd_bias_checks(c, ws, core) : attn_bwd_mask_checks(c, ws, core);
    if (rc != MODCR_OK) return rc;
    const int M = N * S, Mh = N * P;
    char* w = (char*)c.workspace;
    void* qkv = w;
    void* dqkv = w + ws.rows_x;
    void* kvh = P ? w + 2 * ws.rows_x : nullptr;
    void* dkvh = P ? w + 2 * ws.rows_x + ws.rows_h : nullptr;
    // bf16: the weight / input products run on the MFMA path (workspace); fp32 parity path: exact VALU kernels
    void* sub = dtype == MODCR_BF16 ? (void*)(w + 2 * ws.rows_x + 2 * ws.rows_h) : nullptr;
    const int64_t sub_bytes = dtype == MODCR_BF16 ? ws.sub : 0;
    float* stats = (float*)(w + 2 * ws.rows_x + 2 * ws.rows_h + ws.sub);         // (the streaming cores')
    const size_t esz = dtype == MODCR_BF16 ? 2 : 4;
    const void* wkv = (const char*)c.wqkv + (size_t)H * H * esz;                // rows H..3H of wqkv: the K | V projection [2H, H]
    const int32_t rdt = attn_bwd_rows_dtype(core);
    // 1. (with the forward's dump nothing is recomputed: its Q image already holds the chunk means)
    if (!c.dump) {
        rc = modcr_linear_fwd(c.x, H, c.wqkv, H, c.bqkv, nullptr, 0, 0, qkv, 3 * H, M, 3 * H, H, MODCR_ACT_NONE, dtype, rdt, c.stream);
        if (rc != MODCR_OK) return rc;
        if (c.chunk_id) {
            rc = modcr_chunk_mean_q_fwd(qkv, 3 * H, (int64_t)S * 3 * H, c.chunk_id, N, c.chunk_t, H, rdt, c.stream);
            if (rc != MODCR_OK) return rc;
        }
    }
    // 2.
    if (P) {
        rc = modcr_linear_fwd(c.hist, H, wkv, H, c.bqkv + H, nullptr, 0, 0, kvh, 2 * H, Mh, 2 * H, H, MODCR_ACT_NONE, dtype, rdt, c.stream);
        if (rc != MODCR_OK) return rc;
    }
    // 3.
    const hipStream_t st = (hipStream_t)c.stream;
    switch (core) {
    case ATTN_BWD_FIVE: rc = modcr_launch_attn_bwd5(attn_bwd_mask_args(c, core, (float*)qkv, (float*)dqkv), st); break;
    case ATTN_BWD_MFMA: case ATTN_BWD_MFMA_DALIGN: case ATTN_BWD_EXACT:
        rc = modcr_launch_attn_bwd_older(attn_bwd_mask_args(c, core, (float*)qkv, (float*)dqkv), core, dtype, st); break;
    case ATTN_BWD_STREAM: case ATTN_BWD_STREAM_EXACT:
        rc = modcr_launch_attn_long_bwd(attn_bwd_bias_args(c, qkv, dqkv, kvh, dkvh, stats), attn_bwd_core_number(core), dtype, st); break;
    default:                        // ATTN_BWD_BIAS_MFMA, ATTN_BWD_BIAS_EXACT
        rc = modcr_launch_attn_bias_bwd(attn_bwd_bias_args(c, qkv, dqkv, kvh, dkvh, nullptr), attn_bwd_core_number(core), dtype, st); break;
    }
    if (rc != MODCR_OK) return rc;
    // 4.
    if (c.chunk_id) {
        rc = modcr_chunk_mean_q_fwd(dqkv, 3 * H, (int64_t)S * 3 * H, c.chunk_id, N, c.chunk_t, H, rdt, c.stream);
        if (rc != MODCR_OK) return rc;
    }
    // 5.
    rc = modcr_linear_bwd_input_res(dqkv, 3 * H, rdt, c.wqkv, H, c.dx_residual, H, c.dx, H, M, 3 * H, H, dtype, dtype, sub, sub_bytes, c.stream);
    if (rc != MODCR_OK) return rc;
    rc = modcr_linear_bwd_weight(dqkv, 3 * H, rdt, c.x, H, c.dwqkv, c.dbqkv, M, 3 * H, H, c.accumulate, dtype, sub, sub_bytes, c.stream);
    if (rc != MODCR_OK || !P) return rc;
    // 6.
    rc = modcr_linear_bwd_input_res(dkvh, 2 * H, rdt, wkv, H, nullptr, 0, c.d_hist, H, Mh, 2 * H, H, dtype, dtype, sub, sub_bytes, c.stream);
    if (rc != MODCR_OK) return rc;
    return modcr_linear_bwd_weight(dkvh, 2 * H, rdt, c.hist, H, c.dwqkv + (size_t)H * H, c.dbqkv + H, Mh, 2 * H, H, 1, dtype, sub, sub_bytes, c.stream);
}

// the operands every bias-family entry has (hist / d_hist / P: null, null, 0 from modcr_qkv_attn_bias_bwd)
AttnBwdCall attn_bias_call(const char* who, const void* dctx, const void* x, const void* wqkv, const float* bqkv, const float* attn_bias,
                           int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q, const float* head_mask, int64_t head_mask_stride_n,
                           const float* dx_residual, void* dx, float* dwqkv, float* dbqkv, int32_t accumulate, float* d_bias, int32_t N, int32_t S,
                           int32_t H, int32_t A, float attn_p, uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes,
                           int32_t dtype, modcr_stream_t stream) {
    AttnBwdCall c = {};
    c.who = who; c.bias_family = true; c.max_keys = 256;
    c.dctx = dctx; c.x = x; c.wqkv = wqkv; c.bqkv = bqkv; c.bias = attn_bias; c.bias_sn = bias_stride_n; c.bias_sa = bias_stride_a;
    c.bias_sq = bias_stride_q; c.head_mask = head_mask; c.head_mask_sn = head_mask_stride_n; c.dx_residual = dx_residual; c.dx = dx;
    c.dwqkv = dwqkv; c.dbqkv = dbqkv; c.accumulate = accumulate; c.d_bias = d_bias; c.N = N; c.S = S; c.H = H; c.A = A;
    c.attn_p = attn_p; c.seed = seed; c.offset = offset;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.dtype = dtype; c.stream = stream;
    return c;
}

}  // namespace

// ---- the mask family: backward of modcr_qkv_attn_fwd / _dropout_fwd / _lse_fwd / _opt_fwd (no prefix rows) ----
extern "C" int64_t modcr_qkv_attn_bwd_workspace(int32_t N, int32_t S, int32_t H, int32_t dtype) {
    (void)dtype;
    return attn_bwd_ws(N, S, 0, H).bytes();
}

// (the three older entries are modcr_qkv_attn_opt_bwd without its later arguments)
extern "C" int modcr_qkv_attn_bwd(const void* dctx, const void* x, const void* wqkv, const float* bqkv, const float* key_mask,
                                  const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, void* dx, float* dwqkv, float* dbqkv,
                                  int32_t accumulate, int32_t N, int32_t S, int32_t H, int32_t A, void* workspace, int64_t workspace_bytes,
                                  int32_t dtype, modcr_stream_t stream) {
    return modcr_qkv_attn_opt_bwd(dctx, x, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, nullptr, dx, dwqkv, dbqkv, accumulate, N, S, H, A,
                                  0.f, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, workspace, workspace_bytes, dtype, stream);
}

extern "C" int modcr_qkv_attn_dropout_bwd(const void* dctx, const void* x, const void* wqkv, const float* bqkv, const float* key_mask,
                                          const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, const float* dx_residual,
                                          void* dx, float* dwqkv, float* dbqkv, int32_t accumulate, int32_t N, int32_t S, int32_t H, int32_t A,
                                          float attn_p, uint64_t seed, uint64_t offset, const float* d_align, int32_t align_t, void* workspace,
                                          int64_t workspace_bytes, int32_t dtype, modcr_stream_t stream) {
    return modcr_qkv_attn_opt_bwd(dctx, x, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, dx_residual, dx, dwqkv, dbqkv, accumulate, N, S, H,
                                  A, attn_p, seed, offset, d_align, align_t, nullptr, nullptr, nullptr, 0, workspace, workspace_bytes, dtype, stream);
}

extern "C" int modcr_qkv_attn_lse_bwd(const void* dctx, const void* x, const void* wqkv, const float* bqkv, const float* key_mask,
                                      const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, const float* dx_residual, void* dx,
                                      float* dwqkv, float* dbqkv, int32_t accumulate, int32_t N, int32_t S, int32_t H, int32_t A, float attn_p,
                                      uint64_t seed, uint64_t offset, const float* d_align, int32_t align_t, const void* ctx, const float* lse,
                                      const void* qkv_dump, void* workspace, int64_t workspace_bytes, int32_t dtype, modcr_stream_t stream) {
    return modcr_qkv_attn_opt_bwd(dctx, x, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, dx_residual, dx, dwqkv, dbqkv, accumulate, N, S, H,
                                  A, attn_p, seed, offset, d_align, align_t, ctx, lse, qkv_dump, 0, workspace, workspace_bytes, dtype, stream);
}

extern "C" int modcr_qkv_attn_opt_bwd(const void* dctx, const void* x, const void* wqkv, const float* bqkv, const float* key_mask,
                                      const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, const float* dx_residual, void* dx,
                                      float* dwqkv, float* dbqkv, int32_t accumulate, int32_t N, int32_t S, int32_t H, int32_t A, float attn_p,
                                      uint64_t seed, uint64_t offset, const float* d_align, int32_t align_t, const void* ctx, const float* lse,
                                      const void* qkv_dump, int32_t flags, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                      modcr_stream_t stream) {
    AttnBwdCall c = {};
    c.who = "qkv_attn_bwd"; c.max_keys = 256;
    c.dctx = dctx; c.x = x; c.wqkv = wqkv; c.bqkv = bqkv; c.key_mask = key_mask; c.bits = dense_mask_bits; c.chunk_id = chunk_id; c.chunk_t = chunk_t;
    c.dx_residual = dx_residual; c.dx = dx; c.dwqkv = dwqkv; c.dbqkv = dbqkv; c.accumulate = accumulate; c.N = N; c.S = S; c.H = H; c.A = A;
    c.attn_p = attn_p; c.seed = seed; c.offset = offset; c.d_align = d_align; c.align_t = align_t;
    c.ctx = ctx; c.lse = lse; c.dump = qkv_dump; c.flags = flags;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.dtype = dtype; c.stream = stream;
    return attn_bwd(c);
}

// ---- the bias family: backward of modcr_qkv_attn_bias_fwd.  modcr_qkv_attn_bias_bwd: no prefix rows ----
extern "C" int64_t modcr_qkv_attn_bias_bwd_workspace(int32_t N, int32_t S, int32_t H, int32_t dtype) {
    (void)dtype;
    return attn_bwd_ws(N, S, 0, H).bytes();
}

extern "C" int modcr_qkv_attn_bias_bwd_route(int32_t N, int32_t S, int32_t H, int32_t A, int32_t dtype) {
    return attn_bias_bwd_route(N, S, 0, H, A, dtype, 256);
}

extern "C" int modcr_qkv_attn_bias_bwd(const void* dctx, const void* x, const void* wqkv, const float* bqkv, const float* attn_bias,
                                       int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q, const float* head_mask,
                                       int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t, const float* dx_residual, void* dx,
                                       float* dwqkv, float* dbqkv, int32_t accumulate, float* d_bias, int32_t N, int32_t S, int32_t H, int32_t A,
                                       float attn_p, uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                       modcr_stream_t stream) {
    AttnBwdCall c = attn_bias_call("qkv_attn_bias_bwd", dctx, x, wqkv, bqkv, attn_bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask,
                                   head_mask_stride_n, dx_residual, dx, dwqkv, dbqkv, accumulate, d_bias, N, S, H, A, attn_p, seed, offset, workspace,
                                   workspace_bytes, dtype, stream);
    c.chunk_id = chunk_id; c.chunk_t = chunk_t;
    return attn_bwd(c);
}

// ---- modcr_qkv_attn_prefix_bwd: hist [N, P, H], P >= 1 (no chunk mean) ----
extern "C" int64_t modcr_qkv_attn_prefix_bwd_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    (void)dtype;
    return N <= 0 || S <= 0 || P <= 0 || H <= 0 ? 0 : attn_bwd_ws(N, S, P, H).bytes();
}

extern "C" int modcr_qkv_attn_prefix_bwd_route(int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, int32_t dtype) {
    return P <= 0 ? 0 : attn_bias_bwd_route(N, S, P, H, A, dtype, 256);
}

extern "C" int modcr_qkv_attn_prefix_bwd(const void* dctx, const void* x, const void* hist, const void* wqkv, const float* bqkv,
                                         const float* attn_bias, int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q,
                                         const float* head_mask, int64_t head_mask_stride_n, const float* dx_residual, void* dx, void* d_hist,
                                         float* dwqkv, float* dbqkv, int32_t accumulate, float* d_bias, int32_t N, int32_t S, int32_t P, int32_t H,
                                         int32_t A, float attn_p, uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes,
                                         int32_t dtype, modcr_stream_t stream) {
    AttnBwdCall c = attn_bias_call("qkv_attn_prefix_bwd", dctx, x, wqkv, bqkv, attn_bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask,
                                   head_mask_stride_n, dx_residual, dx, dwqkv, dbqkv, accumulate, d_bias, N, S, H, A, attn_p, seed, offset, workspace,
                                   workspace_bytes, dtype, stream);
    c.hist = hist; c.d_hist = d_hist; c.P = P;
    MODCR_REQUIRE(P >= 1 && hist, "%s: no prefix rows (P=%d, hist %s): that call belongs to modcr_qkv_attn_bias_bwd", c.who, P, hist ? "given" : "null");
    return attn_bwd(c);
}

// ---- modcr_qkv_attn_gate_bwd: the two entries above in one (P >= 0), with the gradient of head_mask ----
extern "C" int64_t modcr_qkv_attn_gate_bwd_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    (void)dtype;
    return N <= 0 || S <= 0 || P < 0 || H <= 0 ? 0 : attn_bwd_ws(N, S, P, H).bytes();
}

extern "C" int modcr_qkv_attn_gate_bwd_route(int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, int32_t dtype) {
    return attn_bias_bwd_route(N, S, P, H, A, dtype, 256);
}

extern "C" int modcr_qkv_attn_gate_bwd(const void* dctx, const void* x, const void* hist, const void* wqkv, const float* bqkv,
                                       const float* attn_bias, int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q,
                                       const float* head_mask, int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t,
                                       const float* dx_residual, void* dx, void* d_hist, float* dwqkv, float* dbqkv, int32_t accumulate,
                                       float* d_bias, float* d_head_mask, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                       uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                       modcr_stream_t stream) {
    AttnBwdCall c = attn_bias_call("qkv_attn_gate_bwd", dctx, x, wqkv, bqkv, attn_bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask,
                                   head_mask_stride_n, dx_residual, dx, dwqkv, dbqkv, accumulate, d_bias, N, S, H, A, attn_p, seed, offset, workspace,
                                   workspace_bytes, dtype, stream);
    c.hist = hist; c.d_hist = d_hist; c.P = P; c.chunk_id = chunk_id; c.chunk_t = chunk_t; c.d_head_mask = d_head_mask;
    const int rc = attn_gate_precheck(c);
    return rc != MODCR_OK ? rc : attn_bwd(c);
}

// ---- modcr_qkv_attn_long_bwd: modcr_qkv_attn_gate_bwd with the key limit 512 (opt-in; the streaming cores above 256 keys) ----
extern "C" int64_t modcr_qkv_attn_long_bwd_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    (void)dtype;
    return N <= 0 || S <= 0 || P < 0 || H <= 0 || (int64_t)P + S > 512 ? 0 : attn_bwd_ws(N, S, P, H, 512).bytes();
}

extern "C" int modcr_qkv_attn_long_bwd_route(int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, int32_t dtype) {
    return attn_bias_bwd_route(N, S, P, H, A, dtype, 512);
}

extern "C" int modcr_qkv_attn_long_bwd(const void* dctx, const void* x, const void* hist, const void* wqkv, const float* bqkv,
                                       const float* attn_bias, int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q,
                                       const float* head_mask, int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t,
                                       const float* dx_residual, void* dx, void* d_hist, float* dwqkv, float* dbqkv, int32_t accumulate,
                                       float* d_bias, float* d_head_mask, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                       uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                       modcr_stream_t stream) {
    // at P + S <= 256 this is the gate entry, by its name in the messages too: the key limit does not show there and the workspace is the same;
    // above, step 3 runs the streaming cores (no dropout there) and the workspace grows by their per-row statistics
    AttnBwdCall c = attn_bias_call((int64_t)P + S <= 256 ? "qkv_attn_gate_bwd" : "qkv_attn_long_bwd", dctx, x, wqkv, bqkv, attn_bias, bias_stride_n, bias_stride_a,
                                   bias_stride_q, head_mask, head_mask_stride_n, dx_residual, dx, dwqkv, dbqkv, accumulate, d_bias, N, S, H, A, attn_p,
                                   seed, offset, workspace, workspace_bytes, dtype, stream);
    c.max_keys = 512;
    c.hist = hist; c.d_hist = d_hist; c.P = P; c.chunk_id = chunk_id; c.chunk_t = chunk_t; c.d_head_mask = d_head_mask;
    const int rc = attn_gate_precheck(c);
    return rc != MODCR_OK ? rc : attn_bwd(c);
}

// ---- modcr_qkv_attn_long_drop_bwd: modcr_qkv_attn_long_bwd with attention-probability dropout above 256 keys (opt-in; the DROP cores) ----
extern "C" int64_t modcr_qkv_attn_long_drop_bwd_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    return modcr_qkv_attn_long_bwd_workspace(N, S, P, H, dtype);
}

extern "C" int modcr_qkv_attn_long_drop_bwd_route(int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, int32_t dtype) {
    return attn_bias_bwd_route(N, S, P, H, A, dtype, 512);
}

extern "C" int modcr_qkv_attn_long_drop_bwd(const void* dctx, const void* x, const void* hist, const void* wqkv, const float* bqkv,
                                            const float* attn_bias, int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q,
                                            const float* head_mask, int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t,
                                            const float* dx_residual, void* dx, void* d_hist, float* dwqkv, float* dbqkv, int32_t accumulate,
                                            float* d_bias, float* d_head_mask, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                            uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                            modcr_stream_t stream) {
    // at P + S <= 256 or attn_p = 0 this is modcr_qkv_attn_long_bwd's call, by its names in the messages too; above, step 3 runs the
    // streaming cores' DROP instantiations under the wide counter layout (attn_common.h) -- same workspace, same route
    const bool wide = (int64_t)P + S > 256 && attn_p > 0.f;
    AttnBwdCall c = attn_bias_call(wide ? "qkv_attn_long_drop_bwd" : (int64_t)P + S <= 256 ? "qkv_attn_gate_bwd" : "qkv_attn_long_bwd", dctx, x, wqkv, bqkv,
                                   attn_bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask, head_mask_stride_n, dx_residual, dx, dwqkv, dbqkv,
                                   accumulate, d_bias, N, S, H, A, attn_p, seed, offset, workspace, workspace_bytes, dtype, stream);
    c.max_keys = 512; c.wide_dropout = true;
    c.hist = hist; c.d_hist = d_hist; c.P = P; c.chunk_id = chunk_id; c.chunk_t = chunk_t; c.d_head_mask = d_head_mask;
    const int rc = attn_gate_precheck(c);
    return rc != MODCR_OK ? rc : attn_bwd(c);
}

// ---- modcr_qkv_attn_long_align_bwd: modcr_qkv_attn_long_drop_bwd with dense mask bits and the align map's gradient above 256 keys
// (opt-in; the MASK / DALIGN instantiations of the streaming cores) ----
extern "C" int64_t modcr_qkv_attn_long_align_bwd_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    return modcr_qkv_attn_long_drop_bwd_workspace(N, S, P, H, dtype);
}

extern "C" int modcr_qkv_attn_long_align_bwd_route(int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, int32_t dtype) {
    return modcr_qkv_attn_long_drop_bwd_route(N, S, P, H, A, dtype);
}

extern "C" int modcr_qkv_attn_long_align_bwd(const void* dctx, const void* x, const void* hist, const void* wqkv, const float* bqkv,
                                             const float* attn_bias, int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q,
                                             const float* head_mask, int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t,
                                             const float* dx_residual, void* dx, void* d_hist, float* dwqkv, float* dbqkv, int32_t accumulate,
                                             float* d_bias, float* d_head_mask, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                             uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                             modcr_stream_t stream, const uint32_t* mask_bits, const float* d_align, int32_t align_t,
                                             int32_t flags) {
    const char* who = "qkv_attn_long_align_bwd";
    MODCR_REQUIRE((flags & ~MODCR_ATTN_SIDE_POST_DROPOUT) == 0, "%s: unknown flags 0x%x", who, flags);
    // with neither it is modcr_qkv_attn_long_drop_bwd's call at every key count, by its names in the messages too
    if (!mask_bits && !d_align)
        return modcr_qkv_attn_long_drop_bwd(dctx, x, hist, wqkv, bqkv, attn_bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask,
                                            head_mask_stride_n, chunk_id, chunk_t, dx_residual, dx, d_hist, dwqkv, dbqkv, accumulate, d_bias, d_head_mask,
                                            N, S, P, H, A, attn_p, seed, offset, workspace, workspace_bytes, dtype, stream);
    MODCR_REQUIRE(P == 0 && !hist && !d_hist, "%s: no mask_bits / d_align with prefix rows (P=%d, hist %s, d_hist %s)", who, P, hist ? "given" : "null",
                  d_hist ? "given" : "null");
    if (S <= 256) {
        modcr_set_error("%s: mask_bits / d_align start above 256 keys (S=%d): up to 256 they belong to modcr_qkv_attn_bwd, which serves them "
                        "from lse and the q|k|v dump", who, S);
        return MODCR_ERR_UNSUPPORTED;
    }
    MODCR_REQUIRE(!d_align || (align_t > 0 && align_t < S), "%s: align_t=%d out of range", who, align_t);
    MODCR_REQUIRE(((uintptr_t)mask_bits & 3) == 0 && ((uintptr_t)d_align & 3) == 0, "%s: mask_bits / d_align not 4-byte aligned", who);
    AttnBwdCall c = attn_bias_call(who, dctx, x, wqkv, bqkv, attn_bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask, head_mask_stride_n,
                                   dx_residual, dx, dwqkv, dbqkv, accumulate, d_bias, N, S, H, A, attn_p, seed, offset, workspace, workspace_bytes,
                                   dtype, stream);
    c.max_keys = 512; c.wide_dropout = true;
    c.chunk_id = chunk_id; c.chunk_t = chunk_t; c.d_head_mask = d_head_mask;
    c.bits = mask_bits; c.d_align = d_align; c.align_t = d_align ? align_t : 0; c.flags = flags;
    return attn_bwd(c);
}
