// Fused QKV projection + masked softmax attention for one encoder layer (CDNA4 / gfx950).
//
// bf16 path -- one workgroup per (sequence n, head a), NW = ceil((P+S)/32) rounded to {2,4,6,8}
// waves, wave w owns tile rows / queries 32w..32w+31:
//   phase A  [L_pad x 192] = [prefix;x] . [Wq_a;Wk_a;Wv_a]^T   (K = H, 64-wide K-tiles staged in
//            LDS as swizzled 128-byte rows, v_mfma_f32_32x32x16_bf16).  Q and K are produced with
//            the weights as the MFMA A operand (features in registers, tokens on lanes) so four
//            consecutive features pack into one 8-byte LDS store of a row-major [token][64] image;
//            V is produced the other way round and lands transposed, [64][token], which is what
//            the P.V product wants.  Q, K, V never touch HBM.
//   chunk-mean query (v10:66-78) on the Q image in LDS when chunk_id is given.
//   phase B  S^T = K.Q^T per 32-key tile (keys in registers, query on the lane): the softmax row
//            reduce is a register reduce + one cross-half exchange; the probabilities, converted
//            pairwise to bf16, ARE the B operand of O^T = V^T.P^T (no LDS round trip).
//   epilogue O^T * 1/rowsum -> bf16 -> wave-private LDS transpose -> 128-byte row stores.
// Masks follow the reference: additive -10000 for masked keys inside the sequence
// (modeling_transfomres.py:641), padding lanes beyond P+S are excluded outright.
//
// fp32 path (parity): QKV by the fp32 GEMM into a workspace, chunk-mean kernel, then a plain
// VALU attention core with identical mask semantics.
#include <stdlib.h>

#include <type_traits>

#include <hip/hip_ext.h>

#include "common.h"
#include "attn_common.h"

namespace {

// Measurement hook (modcr_time_next_attn): two hipEvent_t the NEXT fused-attention launch of this thread hands to
// hipExtLaunchKernel, which stamps them at the start and the end of the kernel itself -- the launch's duration as rocprofv3
// reports it.  (A hipEventRecord pair around the call adds the dispatch latency of two extra barrier packets: 5 % on a
// 370 us launch inside a training step.)
thread_local hipEvent_t g_time_start = nullptr, g_time_stop = nullptr;
template <typename K, typename A>
inline void launch_timed(K kernel, dim3 grid, dim3 block, size_t smem, hipStream_t st, const A& args) {
    if (g_time_start && g_time_stop) {
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)smem, st, g_time_start, g_time_stop, 0, args);
        g_time_start = g_time_stop = nullptr;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, smem, st, args);
    }
}

struct AttnArgs {
    const bf16* x; const bf16* hist; const bf16* wqkv; const float* bqkv;
    const float* key_mask; const uint32_t* bits; const int32_t* chunk_id;
    bf16* ctx; float* probs; float* align_map;
    float* lse;     // tile kernels: log2-domain row statistics [N, A, S] for the five-product backward (attn_bwd.hip), or NULL
    bf16* dump;     // tile kernels (two heads per workgroup, no prefix rows): the Q (scaled, chunk-mean applied) | K | V images of
                    // every (sequence, head) as plain rows [N][A][3][LP][64] for the backward (instead of recomputing them), or NULL
    int N, S, P, H, A, chunk_t, align_t;
    int hconc;      // head groups an XCD works on at a time (block -> tile order), 0 = sequence-major
    unsigned long long* trace = nullptr;   // tuning build only (MODCR_ATTN_TRACE_PTR): cycle stamps of workgroup 0's waves 0 and 4 per tile
    int debug;      // tuning build only (MODCR_ATTN_DEBUG, compiled out of the product library): 1 = stop after phase A, 2 = skip the phase-A MFMA loop, 8 = force the exact pass
    // attention-probability dropout (training mode, attn_common.h): on / off; the packed threshold attn_thrm1_2(round(p * 2^16)),
    // the 64-bit key derived from (seed, offset), and 1 / (1 - p)
    int drop_on;
    uint32_t drop_thr2;
    uint64_t drop_key;
    float drop_keep;
    // side outputs (probabilities, align map) AFTER the dropout, P o m / (1 - p), as the reference returns them (modeling_bert.py:69-74,
    // v10:94-106: `attention_probs = self.dropout(attention_probs)` comes before the return) -- MODCR_ATTN_SIDE_POST_DROPOUT; 0 = the
    // un-dropped probabilities (same expectation)
    int side_post_drop;
    // LayerNorm fold PROTOTYPE (tuning library only): x holds the PRE-LayerNorm rows of the previous sublayer,
    // wqkv = bf16(gamma o W), bqkv = d = W beta + b, cfold[3H] = row sums of the folded weights, row_stats[N * L][2] = (rstd, rstd * mu)
    // of every row: the image pass forms rstd * acc - (rstd * mu) * c + d instead of acc + b
#ifdef MODCR_TUNING
    const float* row_stats = nullptr;
    const float* cfold = nullptr;
#endif
    // live-row layout (modcr_qkv_attn_rows_fwd; qkv_attn4_kernel, no prefix rows): sequence n holds only its first
    // L_n = row_start[n + 1] - row_start[n] rows, and they lie back to back from row row_start[n] of x and ctx on.  Tile rows
    // L_n..S-1 (padded regions: keys that every mask hides, queries nobody reads) re-read row L_n - 1 and are not stored; masks, chunk
    // ids, the align map and the dropout counters stay indexed by (n, s).  NULL = the dense [N, S, H] layout.
    const int32_t* row_start = nullptr;
};

constexpr int VT_PAD = 8;  // bytes of padding per V^T row: stride/4 = 2*odd -> conflict-free b64 reads

// HPW = heads per workgroup.  A 6-wave workgroup (S <= 192) lands 2,2,1,1 on the four SIMDs and a
// second one only fits beside it if the dispatcher happens to rotate its start SIMD -- measured
// residency was ~1 workgroup per CU.  Two heads of the same sequence per workgroup give 12 waves
// = 3 per SIMD by construction, share the X tile of the QKV GEMM (half the L2->LDS traffic for X)
// and let one wave's softmax VALU run under its SIMD neighbours' MFMAs.
// OCC = minimum waves per SIMD the register allocator must leave room for.
// BKA / NSLOT: K-tile width (64 = full 128-byte lines, 32) and ring depth of the phase-A staging.
template <int NW, int HPW, int OCC, int BKA, int NSLOT>
__global__ __launch_bounds__(NW * HPW * 64, OCC) void qkv_attn_bf16_kernel(AttnArgs p) {
    constexpr int LP = NW * 32;              // padded key / tile-row count
    constexpr int NTH = NW * 64;             // threads per head
    constexpr int NT = NTH * HPW;            // threads
    constexpr int VT_STRIDE = LP * 2 + VT_PAD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // phase A view: two ring slots of {X tile: LP rows x 128 B, W tile per head: 192 rows x 128 B}
    // phase B view (aliases phase A after a barrier)
    constexpr int ROWB = BKA * 2;                // bytes per staged row
    constexpr int STAGE = (LP + 192 * HPW) * ROWB; // bytes per ring slot: X tile + one W tile per head
    constexpr int END_A = NSLOT * STAGE, HEAD_B = 2 * LP * 128 + 64 * VT_STRIDE, END_B = HPW * HEAD_B;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hd = wave_all / NW, wave = wave_all % NW;   // head within the workgroup, wave within the head
    const int ltid = tid - hd * NTH;
    unsigned char* sQ = smem + hd * HEAD_B;      // LP x 128 B, row = query index
    unsigned char* sK = sQ + LP * 128;           // LP x 128 B, row = key index
    unsigned char* sVt = sQ + 2 * LP * 128;      // 64 rows x VT_STRIDE
    float* sMask = reinterpret_cast<float*>(smem + (END_A > END_B ? END_A : END_B));  // LP floats, outside both views
    float* sBiasAll = sMask + LP;                                                     // 192 floats per head
    int* sCid = reinterpret_cast<int*>(sBiasAll + 192 * HPW);                         // LP ints
    float* sBias = sBiasAll + hd * 192;

    const int hgroups = p.A / HPW;
    const int nwg = p.N * hgroups;
    // Block -> (sequence, head group).  Blocks go round-robin over the 8 XCDs; each XCD owns a
    // contiguous run of sequences.  Inside an XCD the order is head-group-major over `hconc` groups at
    // a time, so the ~32 workgroups resident on the XCD share hconc weight slices (hconc x 576 KiB,
    // L2-resident) instead of all of Wqkv (3.4 MiB of the 4 MiB L2, evicted by the X stream).
    int n, hg;
    if (p.hconc > 0 && (p.N & 7) == 0) {
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, ns = p.N >> 3, G = p.hconc;
        const int hgb = idx / (ns * G), rem = idx - hgb * ns * G;
        const int gw = min(G, hgroups - hgb * G);          // last block of groups may be narrower
        n = xcd * ns + rem / gw;
        hg = hgb * G + rem % gw;
    } else {
        const int tile = xcd_remap(blockIdx.x, nwg);
        n = tile / hgroups, hg = tile % hgroups;
    }
    const int a0 = hg * HPW, a = a0 + hd;
    const int r = lane & 31, h = lane >> 5;
    const int S = p.S, P = p.P, L = P + S, H = p.H;

    // ---- small per-block tables ------------------------------------------------------------
    for (int j = tid; j < LP; j += NT) {
        // scores are kept in the log2 domain (Q is scaled by log2(e)/8), so the additive mask is too
        float m;
        if (j >= L) m = -INFINITY;
        else if (p.bits) m = 0.f;
        else m = (1.0f - p.key_mask[(int64_t)n * L + j]) * (MODCR_NEG * LOG2E);
        sMask[j] = m;
        sCid[j] = (p.chunk_id && j < p.chunk_t) ? p.chunk_id[(int64_t)n * p.chunk_t + j] : -1;
    }
    for (int j = tid; j < 192 * HPW; j += NT) {
        const int jh = j / 192, jj = j % 192;
        sBiasAll[j] = p.bqkv[(jj >> 6) * H + (a0 + jh) * 64 + (jj & 63)];
    }

    // ---- phase A: QKV tile GEMM ---------------------------------------------------------------
    // [LP tokens] x [192 features per head] over K = H.  K-tiles of 64 (128-byte rows) arrive by
    // LDS-DMA (8 rows = 1 KiB per instruction) into a two-slot ring: the DMA of tile k+1 is issued
    // right after the barrier that opens tile k and lands while tile k feeds the MFMAs.  LDS is
    // written linearly, so the XOR swizzle (slot s of row r holds logical chunk s ^ ((r>>1)&7))
    // is applied to the SOURCE address.  Within a head, wave w owns token blocks {2(w/2), 2(w/2)+1}
    // x feature blocks {3(w%2) .. 3(w%2)+2}: 5 fragment reads per 6 MFMAs.
    constexpr int NWAVES = NW * HPW;
    constexpr int RPC = 1024 / ROWB;            // rows per 1-KiB DMA piece (8 or 16)
    constexpr int CPRW = ROWB / 16;             // 16-byte chunks per row (8 or 4)
    constexpr int XCH = LP / RPC;               // pieces of the X tile
    constexpr int WCHH = 192 / RPC;             // pieces of one head's W tile
    constexpr int NCH = XCH + WCHH * HPW;
    constexpr int CPW = NCH / NWAVES;           // pieces (DMA instructions) per wave per K-tile
    static_assert(NCH % NWAVES == 0, "pieces must divide evenly over the waves");
    static_assert(STAGE == NCH * 1024, "stage size");
    static_assert((NSLOT - 1) * CPW < 64, "vmcnt field");
    auto skey = [](int row) { return BKA == 64 ? (row >> 1) & 7 : (row >> 2) & 3; };
    auto soff = [](int row, int chunk) {
        return BKA == 64 ? (row << 7) + (((chunk ^ (row >> 1)) & 7) << 4) : (row << 6) + (((chunk ^ (row >> 2)) & 3) << 4);
    };
    const bf16* gsrc[CPW];
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
        const int id = wave_all + q * NWAVES;
        if (id < XCH) {
            const int trow = id * RPC + lane / CPRW;
            const int row = min(trow, L - 1);                                // padding rows re-read row L-1
            const int c = (lane % CPRW) ^ skey(trow);
            const bf16* base = (row < P) ? p.hist + ((int64_t)n * P + row) * H
                                         : p.x + ((int64_t)n * S + (row - P)) * H;
            gsrc[q] = base + c * 8;
        } else {
            const int w = id - XCH, wh = w / WCHH;
            const int f = (w % WCHH) * RPC + lane / CPRW;                    // 0..191 = q|k|v feature of head a0+wh
            const int c = (lane % CPRW) ^ skey(f);
            gsrc[q] = p.wqkv + ((int64_t)(f >> 6) * H + (a0 + wh) * 64 + (f & 63)) * H + c * 8;
        }
    }
    auto stage = [&](int buf, int k0) {
#pragma unroll
        for (int q = 0; q < CPW; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(gsrc[q] + k0),
                                             (lptr_t)(smem + buf * STAGE + (wave_all + q * NWAVES) * 1024), 16, 0, 0);
    };

    const int tg = wave >> 1, fg = wave & 1;
    f32x16 acc[2][3];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][j][e] = 0.f;

    // Ring of NSLOT K-tiles with NSLOT-1 in flight: top of iteration kt waits (counted vmcnt) until
    // tile kt has landed, raw barrier, refill of the slot everyone finished reading one iteration
    // ago, compute.  LDS-DMA pieces land ~1-2 us after issue, a K-tile computes in ~1 us: one tile in
    // flight leaves the matrix pipe waiting for data.
    constexpr int PRE = NSLOT - 1;
    constexpr int KSTEPS = BKA / 16;
    const int nk = MODCR_DBG(p.debug & 2) ? 0 : (H / BKA);
    auto gemm_loop = [&](auto FG) {
        constexpr int fgc = decltype(FG)::value;
#pragma unroll
        for (int t = 0; t < PRE; ++t)
            if (t < nk) stage(t, t * BKA);
        for (int kt = 0; kt < nk; ++kt) {
            const int rem = nk - 1 - kt;                    // tiles issued after kt
            if (rem >= PRE - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((PRE - 1) * CPW) : "memory");
            else if (PRE >= 3 && rem == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (kt + PRE < nk && !MODCR_DBG(p.debug & 4)) stage((kt + PRE) % NSLOT, (kt + PRE) * BKA);   // debug bit2: timing-only, no refill
            const unsigned char* sXs = smem + (kt % NSLOT) * STAGE;
            const unsigned char* sWs = sXs + (XCH + WCHH * hd) * 1024;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                bf16x8 fx[2], fw[3];
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    fx[t] = *reinterpret_cast<const bf16x8*>(sXs + soff((2 * tg + t) * 32 + r, ks * 2 + h));
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    fw[j] = *reinterpret_cast<const bf16x8*>(sWs + soff((3 * fgc + j) * 32 + r, ks * 2 + h));
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (fgc == 0 || j == 0)   // Q, K: features in registers, tokens on lanes
                            acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[j], fx[t], acc[t][j], 0, 0, 0);
                        else                      // V: tokens in registers, features on lanes
                            acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fx[t], fw[j], acc[t][j], 0, 0, 0);
                    }
            }
        }
    };
    if (fg == 0) gemm_loop(std::integral_constant<int, 0>{});
    else gemm_loop(std::integral_constant<int, 1>{});
    __syncthreads();        // every wave is done with the staging ring before it becomes the Q/K/V images

    // ---- write Q (scaled by 1/8), K, V^T (+bias) as bf16 images into LDS ----------------------
    auto put_feat = [&](const f32x16& v16, int trow, int fbase, bool isq) {
        // features fbase + 8g + 4h + e in the registers, token row `trow` on this lane
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int f0 = fbase + 8 * g + 4 * h;
            bf16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = v16[4 * g + e] + sBias[(isq ? 0 : 64) + f0 + e];
                if (isq) t *= 0.125f * LOG2E;
                v[e] = (bf16)t;
            }
            if (isq) {
                const int qi = trow - P;
                if (qi >= 0) *reinterpret_cast<bf16x4*>(sQ + swz128(qi, f0 >> 3) + (f0 & 7) * 2) = v;
            } else {
                *reinterpret_cast<bf16x4*>(sK + swz128(trow, f0 >> 3) + (f0 & 7) * 2) = v;
            }
        }
    };
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int tb = (2 * tg + t) * 32;
        if (fg == 0) {
            put_feat(acc[t][0], tb + r, 0, true);
            put_feat(acc[t][1], tb + r, 32, true);
            put_feat(acc[t][2], tb + r, 0, false);
        } else {
            put_feat(acc[t][0], tb + r, 32, false);
#pragma unroll
            for (int j = 1; j < 3; ++j) {
                const int f = (j - 1) * 32 + r;
                const float bv = sBias[128 + f];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int t0 = tb + 8 * g + 4 * h;       // first of 4 consecutive tokens
                    bf16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (bf16)(acc[t][j][4 * g + e] + bv);
                    *reinterpret_cast<bf16x4*>(sVt + f * VT_STRIDE + t0 * 2) = v;
                }
            }
        }
    }
    __syncthreads();

    // ---- chunk-mean query (phase-3 layers of seq_enc) ----------------------------------------
    if (p.chunk_id) {
        const int T = p.chunk_t;
        bf16x4 mean[8];
        bool have[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int item = ltid + NTH * it;
            const int t = item >> 4, c4 = item & 15;
            have[it] = false;
            if (t < T) {
                const int id = sCid[t];
                if (id >= 0) {
                    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                    int cnt = 0;
                    for (int u = 0; u < T; ++u) {
                        if (sCid[u] == id) {
                            const bf16x4 q = *reinterpret_cast<const bf16x4*>(sQ + swz128(u, c4 >> 1) + (c4 & 1) * 8);
                            s0 += (float)q[0]; s1 += (float)q[1]; s2 += (float)q[2]; s3 += (float)q[3];
                            ++cnt;
                        }
                    }
                    const float inv = 1.0f / (float)cnt;
                    mean[it][0] = (bf16)(s0 * inv); mean[it][1] = (bf16)(s1 * inv);
                    mean[it][2] = (bf16)(s2 * inv); mean[it][3] = (bf16)(s3 * inv);
                    have[it] = true;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int item = ltid + NTH * it;
            const int t = item >> 4, c4 = item & 15;
            if (have[it]) *reinterpret_cast<bf16x4*>(sQ + swz128(t, c4 >> 1) + (c4 & 1) * 8) = mean[it];
        }
        __syncthreads();
    }

    if (MODCR_DBG(p.debug & 1)) return;
    // ---- phase B: per 32-key tile S^T = K.Q^T -> online softmax -> O^T += V^T.P^T ---------------
    // Keys of a tile sit in the 16 accumulator registers (key = 32kt + (e&3) + 8(e>>2) + 4h), the
    // query on the lane: the row max / sum are register reductions plus one exchange with lane^32,
    // and the exponentiated tile, converted pairwise to bf16, is the B operand of the P.V MFMA.
    const int q0 = wave * 32;
    const int qi = q0 + r;                                  // this lane's query
    const int LW = (L + 31) >> 5;
    bf16x8 fq[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        fq[ks] = *reinterpret_cast<const bf16x8*>(sQ + swz128(qi, ks * 2 + h));

    auto score_tile = [&](int kt, f32x16& sc) {             // masked log2-domain scores of key tile kt
        // the accumulator starts from the additive mask (0 / -10000*log2e / -inf for tile padding), so
        // masking costs no VALU pass after the MFMAs
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + kt * 32 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) sc[4 * g + e] = mk[e];
        }
        if (p.bits) {                                       // dense mask: bit (8g+4h+e) of this query's word
            const uint32_t word = (qi < S && kt * 32 < L) ? p.bits[((int64_t)n * S + qi) * LW + kt] : 0xffffffffu;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!((word >> (8 * (e >> 2) + 4 * h + (e & 3))) & 1u)) sc[e] += MODCR_NEG * LOG2E;
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 fk = *reinterpret_cast<const bf16x8*>(sK + swz128(kt * 32 + r, ks * 2 + h));
            sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fk, fq[ks], sc, 0, 0, 0);
        }
    };

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NW; ++kt) {
        if (kt * 32 >= L) break;                            // block-uniform: tile holds padding only
        f32x16 sc;
        score_tile(kt, sc);
        float tmax = sc[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) tmax = fmaxf(tmax, sc[e]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);             // finite: tile 0 always holds key 0 < L
        float lsum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float ex = __builtin_amdgcn_exp2f(sc[e] - m_new);
            sc[e] = ex;
            lsum += ex;
        }
        if (__any(m_new > m_run)) {                         // wave-uniform: some row's max moved -> rescale
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
        }
        l_run += lsum;
        m_run = m_new;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 pb;
#pragma unroll
            for (int j = 0; j < 8; ++j) pb[j] = (bf16)sc[8 * s2 + j];
            if (p.drop_on) {
                // attention-probability dropout (training mode; the row sum above took the unmasked weights): registers
                // 0-3 / 4-7 of pb are keys 32 kt + 16 s2 + 4 h + 0..3 and + 8, i.e. the l4 groups h and h + 2 of the 16-key
                // block 2 kt + s2 of this lane's query (mask layout: attn_common.h)
                u32x4_t w = __builtin_bit_cast(u32x4_t, pb);
                const uint32_t row = (uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qi);
                const uint32_t b0 = attn_drop_base(row, (uint32_t)h, p.drop_key), b1 = attn_drop_base(row, (uint32_t)(h + 2), p.drop_key);
                const int j0 = (2 * kt + s2) * 2;
                w[0] &= attn_keep2(attn_drop_word(b0, j0, p.drop_key), p.drop_thr2);
                w[1] &= attn_keep2(attn_drop_word(b0, j0 + 1, p.drop_key), p.drop_thr2);
                w[2] &= attn_keep2(attn_drop_word(b1, j0, p.drop_key), p.drop_thr2);
                w[3] &= attn_keep2(attn_drop_word(b1, j0 + 1, p.drop_key), p.drop_thr2);
                pb = __builtin_bit_cast(bf16x8, w);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const unsigned char* vrow = sVt + (dt * 32 + r) * VT_STRIDE + (kt * 32 + 16 * s2 + 4 * h) * 2;
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow);
                const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vrow + 16);
                bf16x8 va;
                va[0] = lo[0]; va[1] = lo[1]; va[2] = lo[2]; va[3] = lo[3];
                va[4] = hi[0]; va[5] = hi[1]; va[6] = hi[2]; va[7] = hi[3];
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o[dt], 0, 0, 0);
            }
        }
    }
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));
    const float inv_ctx = p.drop_on ? inv * p.drop_keep : inv;              // context rows carry dropout's 1 / (1 - p)

    // optional side outputs (parity tests, align-loss layers): recompute each tile against the
    // final row max / sum
    if (p.probs || p.align_map) {
        float* pr = (p.probs && qi < S) ? p.probs + (((int64_t)n * p.A + a) * S + qi) * L : nullptr;
        const bool amap = p.align_map && q0 < p.align_t;                 // wave-uniform
        const int T = p.align_t, R = S - T;
        float* sS = reinterpret_cast<float*>(sQ + q0 * 128);             // this wave's own 4 KB (Q rows are in registers)
#pragma unroll
        for (int kt = 0; kt < NW; ++kt) {
            if (kt * 32 >= L) break;
            f32x16 sc;
            score_tile(kt, sc);
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = __builtin_amdgcn_exp2f(sc[e] - m_run) * inv;
            if (pr) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (key < L) pr[key] = sc[e];
                }
            }
            if (amap && kt * 32 + 31 >= P + T) {                          // tile holds region keys
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int c = (e & 3) + 8 * (e >> 2) + 4 * h;
                    sS[r * 32 + (c ^ r)] = sc[e];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int row = it * 2 + h, col = r;
                    const int key = kt * 32 + col, q = q0 + row;
                    const float v = sS[row * 32 + (col ^ row)];
                    if (q < T && key >= P + T && key < L)
                        atomicAdd(p.align_map + ((int64_t)n * T + q) * R + (key - P - T), v);
                }
            }
        }
    }

    // epilogue: normalise, transpose through this wave's private 4 KB, store 128-byte rows
    {
        unsigned char* sO = sQ + q0 * 128;       // rows q0..q0+31, 128 B each, plain (unswizzled)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (bf16)(o[dt][4 * g + e] * inv_ctx);
                const int d0 = dt * 32 + 8 * g + 4 * h;
                *reinterpret_cast<bf16x4*>(sO + r * 128 + ((((d0 >> 3) ^ r) & 7) << 4) + (d0 & 7) * 2) = v;
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = it * 8 + (lane >> 3), ch = lane & 7;
            const uint4 v = *reinterpret_cast<const uint4*>(sO + row * 128 + (((ch ^ row) & 7) << 4));
            const int q = q0 + row;
            if (q < S)
                *reinterpret_cast<uint4*>(p.ctx + ((int64_t)n * S + q) * H + a * 64 + ch * 8) = v;
        }
    }
}

template <int NW, int HPW, int BKA, int NSLOT> constexpr size_t attn_smem_bytes() {
    constexpr int LP = NW * 32;
    constexpr size_t end_a = (size_t)NSLOT * (LP + 192 * HPW) * BKA * 2;
    constexpr size_t end_b = (size_t)HPW * (2 * LP * 128 + 64 * (LP * 2 + VT_PAD));
    return (end_a > end_b ? end_a : end_b) + (size_t)LP * 4 + 192 * HPW * 4 + (size_t)LP * 4;
}

template <int NW, int HPW, int OCC, int BKA, int NSLOT>
int launch_attn(const AttnArgs& p, hipStream_t st) {
    static bool configured_dev[MODCR_MAX_DEV] = {};
    bool& configured = configured_dev[modcr_device_index()];   // idempotent attribute set; benign if raced
    const size_t smem = attn_smem_bytes<NW, HPW, BKA, NSLOT>();
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qkv_attn_bf16_kernel<NW, HPW, OCC, BKA, NSLOT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) {
            modcr_set_error("qkv_attn: cannot reserve %zu bytes of LDS: %s", smem, hipGetErrorString(e));
            return MODCR_ERR_LAUNCH;
        }
        configured = true;
    }
    launch_timed(qkv_attn_bf16_kernel<NW, HPW, OCC, BKA, NSLOT>, dim3(p.N * (p.A / HPW)), dim3(NW * HPW * 64), smem, st, p);
    return modcr_check_launch("qkv_attn_bf16");
}

// ---- v4: 8 waves in two staggered groups, half-tile ring (the GEMM's 8-phase schedule) ----------
// One workgroup = one sequence x two heads, 128 < S <= 192, no prefix.
//   phase A  [192 tokens] x [384 features = (q|k|v) of two heads] over K = H on the schedule of
//            linear_bf16_p8_kernel (gemm.hip): K-tiles of 64 split into four half-tiles {A0, B0, B1, A1}
//            (A = 96 token rows = 12 KB: rows wr*48.. of both wave rows; B = 192 feature rows = 24 KB),
//            one half-tile staged per phase six phases ahead by LDS-DMA, counted vmcnt that leaves four
//            half-tiles (10 DMA instructions per wave) in flight, 18 v_mfma_f32_16x16x32_bf16 between
//            two raw barriers; the wave groups wr = 0 / 1 (one wave of each per SIMD) run one barrier
//            apart.  Wave (wr, wc) owns tokens wr*96.. x {64 features of q or k of head wc>>1, 32 features
//            of v of head wc>>1}: q/k blocks are produced with the weights as the MFMA A operand
//            (4 consecutive features per lane -> 8-byte stores into the row-major [token][64] images),
//            v blocks the other way round ([64][token] image).
//   phase B  wave = (head, 48 queries).  S^T = K.Q^T for all 192 keys stays in registers (the 144
//            accumulator registers of phase A), the additive mask is the MFMA accumulator init, so the
//            row max is exact: one pass, no rescale, two cross-lane steps per 16 queries in total.
//            P = exp2(S - max) in place, bf16 pairs of two 16-key blocks are the B operand of
//            O^T += V^T.P^T (keys permuted identically on the V^T fragment reads).
// NH = heads per workgroup: 2 for the token tiles 128 and 192 (64 < S <= 192); 1 for the 256-token tile (192 < S <= 256, the
// VCR / Oscar-large shape class S = 230): two heads' Q | K | V^T images of 256 tokens do not fit the 160 KB of LDS.  The 8 waves
// of phase A form WR wave rows x WC wave columns (a wave column = 96 features: q or k of a head + half of its v), i.e.
// 2 x 4 (NH = 2) or 4 x 2 (NH = 1); phase B gives every head 8 / NH waves of QW queries each.
template <int LP_, int NH_ = 2>
struct A4T {
    static constexpr int LP = LP_, NH = NH_, NF = 192 * NH, NT = 512;   // token tile, heads, features (q|k|v of NH heads)
    static constexpr int WC = 2 * NH, WR = 8 / WC;              // wave grid of phase A
    static constexpr int RW = LP / WR;                          // tokens per wave row
    static constexpr int QW = RW / 2;                           // tokens per (wave row, half) = queries per wave in phase B
    static constexpr int NI = QW / 16;                          // 16-token blocks per (wave row, half)
    static constexpr int NQB = QW / 16, NKT = LP / 32;          // query blocks per wave, 32-key tiles
    static constexpr int WPH = 8 / NH;                          // waves per head in phase B
    static constexpr int NA = (LP / 2 > 64) ? 2 : 1;            // LDS-DMA instructions per wave per A half (LP = 192: the 2nd by lanes 0..31)
    static constexpr bool A_HALF_PIECE = (LP / 2) % 64 != 0;    // the 2nd A instruction moves half a piece (4 rows per wave)
    static constexpr int NBI = NH == 2 ? 3 : 2;                 // ... per B half (NH = 1: one piece + half a piece by lanes 0..31)
    static constexpr int HA = (LP / 2) * 128, HB = (NF / 2) * 128;   // bytes per half-tile
    static constexpr int KT = 2 * HA + 2 * HB;                  // A0 | A1 | B0 | B1
    static constexpr int RING = 2 * KT;
    static constexpr int VT_STRIDE = LP * 2 + VT_PAD;
    static constexpr int IMGS = 2 * NH * LP * 128 + NH * 64 * VT_STRIDE;
    static constexpr int MAIN = (IMGS > RING) ? IMGS : RING;
    static constexpr int DROP_OFF = MAIN + LP * 4 + NF * 4 + LP * 4 + 16 + 3 * LP * 4;   // 8 dwords: attention-dropout parameters, P
    static constexpr int SMEM = DROP_OFF + 48;                  // + 3 dwords: first context row of the tile's sequence (64 bit), its row count
    static constexpr int FOLD_OFF = SMEM;                       // FOLD variants: sRs[LP] | sRm[LP] | sC[NF] floats behind everything else
    static constexpr int SMEM_FOLD = FOLD_OFF + 2 * LP * 4 + NF * 4;
    static constexpr int FLY4 = 2 * NA + 2 * NBI;               // DMA instructions per wave in four consecutive half-tiles
    // phase-B images over the ring: [Q0 | Q1 | K0 | K1 | Vt0 | Vt1]  (NH = 1: [Q | K | Vt])
    static __device__ __forceinline__ unsigned char* img_qk(unsigned char* smem, int part, int head) { return smem + (part * NH + head) * LP * 128; }
    static __device__ __forceinline__ unsigned char* img_vt(unsigned char* smem, int head) { return smem + 2 * NH * LP * 128 + head * 64 * VT_STRIDE; }
};
typedef A4T<192> A4;

// epilogue of one wave: O^T / rowsum -> bf16 -> transposed through the wave's own 48 Q rows -> 128-byte row stores
// rows [row_lo, row_hi) of the wave's 48 / 32 tile rows are query rows of the sequence (prefix rows in front and the padded
// tail behind are not); ctx_rows points at the output row of tile row 0 of the wave (possibly before the sequence: masked)
template <typename A4>
__device__ __forceinline__ void attn4_store_ctx(const f32x4 (&o)[4][A4::NQB], const float (&inv)[A4::NQB], unsigned char* sO, bf16* ctx_rows,
                                                int H, int row_lo, int row_hi, int l15, int l4, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
    for (int qb = 0; qb < A4::NQB; ++qb)
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            bf16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (bf16)(o[db][qb][e] * inv[qb]);
            const int row = qb * 16 + l15, d0 = db * 16 + 4 * l4;
            *reinterpret_cast<bf16x4*>(sO + row * 128 + ((((d0 >> 3) ^ row) & 7) << 4) + (d0 & 7) * 2) = v;
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#pragma unroll
    for (int it = 0; it < A4::QW / 8; ++it) {
        const int row = it * 8 + (lane >> 3), ch = lane & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(sO + row * 128 + (((ch ^ row) & 7) << 4));
        if (row >= row_lo && row < row_hi) *reinterpret_cast<uint4*>(ctx_rows + (int64_t)row * H + ch * 8) = v;
    }
}

// Chunk-mean queries (v10:66-78) on the Q images of both heads, for the whole workgroup (contains barriers).
// Out of line: its twelve unrolled items would otherwise shape the register allocation of the kernel around it.
template <int LP, int NH>
__device__ __attribute__((noinline)) void attn4_chunk_mean(unsigned char* smem, int T, int tid) {
    typedef A4T<LP, NH> A4;                                 // NH = 2: 256 threads per head; NH = 1: all 512 on the one head
    constexpr int TPH = A4::NT / NH, ITS = LP * 16 / TPH;
    float* sMask = reinterpret_cast<float*>(smem + A4::MAIN);
    int* sCid = reinterpret_cast<int*>(sMask + LP + A4::NF);
    int* sFlag = sCid + LP;
    int* sFirst = sFlag + 4;
    int* sLast = sFirst + LP;
    int* sCnt = sLast + LP;
    unsigned char* sQ = A4::img_qk(smem, 0, tid / TPH);
    const int ltid = tid % TPH;
    // first / last token and size of every chunk id; when each chunk is one contiguous run of tokens (the
    // data format: utils/GetChunk_v4_vcr.py offsets are consecutive token indices) a token's mean is a sum over
    // [first, last] instead of a scan of all T tokens.  Anything else takes the scan.
    if (tid < T) {
        const int id = sCid[tid];
        if (id >= LP) sFlag[1] = 1;
        else if (id >= 0) { atomicMin(&sFirst[id], tid); atomicMax(&sLast[id], tid); atomicAdd(&sCnt[id], 1); }
    }
    __syncthreads();
    if (tid < LP && sCnt[tid] > 0 && sLast[tid] - sFirst[tid] + 1 != sCnt[tid]) sFlag[1] = 1;
    __syncthreads();
    const bool runs = sFlag[1] == 0;
    bf16x4 mean[ITS];
    bool have[ITS];
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
        const int item = ltid + TPH * it;
        const int t = item >> 4, c4 = item & 15;
        have[it] = false;
        if (t < T) {
            const int id = sCid[t];
            if (id >= 0) {
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                int cnt = 0;
                const int u0 = runs ? sFirst[id] : 0, u1 = runs ? sLast[id] + 1 : T;
                for (int u = u0; u < u1; ++u) {
                    if (sCid[u] == id) {
                        const bf16x4 q = *reinterpret_cast<const bf16x4*>(sQ + swz128(u, c4 >> 1) + (c4 & 1) * 8);
                        s0 += (float)q[0]; s1 += (float)q[1]; s2 += (float)q[2]; s3 += (float)q[3];
                        ++cnt;
                    }
                }
                const float inv = 1.0f / (float)cnt;
                mean[it][0] = (bf16)(s0 * inv); mean[it][1] = (bf16)(s1 * inv);
                mean[it][2] = (bf16)(s2 * inv); mean[it][3] = (bf16)(s3 * inv);
                have[it] = true;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
        const int item = ltid + TPH * it;
        const int t = item >> 4, c4 = item & 15;
        if (have[it]) *reinterpret_cast<bf16x4*>(sQ + swz128(t, c4 >> 1) + (c4 & 1) * 8) = mean[it];
    }
    __syncthreads();
}

// Exact phase B of one tile for the whole workgroup (all 8 waves call it together: it contains barriers): all 192
// scores of a row in registers, exact row max, optional probabilities / head-summed text->region map, context
// store.  The generic variant (MODE 0) always runs it; the production variants only when the streaming pass
// found a row sum out of range, so it is kept out of line (its 144 score registers would otherwise shape the
// register allocation of the hot path).
template <int LP, int NH>
__device__ __attribute__((noinline)) void attn4_exact_tail(unsigned char* smem, const uint32_t* bits, float* probs, float* align_map,
                                                           bf16* ctx, int align_t, int S, int H, int A, int n, int a0, int tid) {
    // (prefix rows: P rides in the LDS parameter block, see sDrop[4]; S = query rows, L = P + S keys / tile rows)
    typedef A4T<LP, NH> A4;
    // attention-dropout parameters: left in LDS by the kernel (more call arguments change how the CALLER's accumulators
    // are kept around the call: measured 100 MB of scratch traffic per launch on the common path)
    const uint32_t* sDrop = reinterpret_cast<const uint32_t*>(smem + A4::DROP_OFF);
    const uint32_t drop_thr2 = sDrop[0];
    const uint64_t drop_key = ((uint64_t)sDrop[2] << 32) | sDrop[1];
    const float drop_keep = __uint_as_float(sDrop[3]);
    const bool drop_on = drop_keep != 1.0f;                 // the kernel leaves 1.0 there when the masking is off
    const int P = (int)sDrop[4];
    float* lse_out = reinterpret_cast<float*>(((uint64_t)sDrop[6] << 32) | sDrop[5]);
    const bool side_post = drop_on && sDrop[7] != 0;        // probabilities / align map after the dropout (reference semantics)
    const int64_t crow = (int64_t)(((uint64_t)sDrop[9] << 32) | sDrop[8]);      // first context row of sequence n (n * S, or row_start[n])
    const int Ln = (int)sDrop[10];                          // tile rows of the sequence that exist (P + S, or the live-row count)
    const int thr_s = (int)(short)(drop_thr2 & 0xffffu) + 1;   // signed 16-bit threshold: kept iff field >= thr_s
    constexpr int VT_STRIDE = A4::VT_STRIDE, NKT = A4::NKT, NQB = A4::NQB;
    const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int hd = wave / A4::WPH, qbase = (wave % A4::WPH) * A4::QW, a = a0 + hd, L = P + S;
    const int LW = (L + 31) >> 5;
    const float* sMask = reinterpret_cast<const float*>(smem + A4::MAIN);
    const unsigned char* sQ = A4::img_qk(smem, 0, hd);
    const unsigned char* sK = A4::img_qk(smem, 1, hd);
    const unsigned char* sVt = A4::img_vt(smem, hd);
    f32x4 sc[NKT][NQB][2];
    {
        bf16x8 fq[NQB][2];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                fq[qb][ks] = *reinterpret_cast<const bf16x8*>(sQ + swz128(qbase + qb * 16 + l15, ks * 4 + l4));
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int krow = kt * 32 + kb * 16;
                const bf16x8 fk0 = *reinterpret_cast<const bf16x8*>(sK + swz128(krow + l15, l4));
                const bf16x8 fk1 = *reinterpret_cast<const bf16x8*>(sK + swz128(krow + l15, 4 + l4));
                const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + krow + 4 * l4);
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) {
                    f32x4 c = mk;
                    if (bits) {                             // dense mask: bit (16 kb + 4 l4 + e) of this query's word
                        const int qi = qbase + qb * 16 + l15 - P;
                        const uint32_t word = (qi >= 0 && qi < S && kt < LW) ? bits[((int64_t)n * S + qi) * LW + kt] : 0xffffffffu;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (!((word >> (kb * 16 + 4 * l4 + e)) & 1u)) c[e] += MODCR_NEG * LOG2E;
                    }
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk0, fq[qb][0], c, 0, 0, 0);
                    sc[kt][qb][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk1, fq[qb][1], c, 0, 0, 0);
                }
            }
    }
    uint32_t dbase[NQB];                                    // dropout bases of this lane's query rows (attn_common.h)
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) dbase[qb] = attn_drop_base((uint32_t)((n * A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qbase + qb * 16 + l15 - P), (uint32_t)l4, drop_key);
    float mx[NQB], ls[NQB], inv[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) m = fmaxf(m, sc[kt][qb][kb][e]);
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));                // finite: key 0 < L
        mx[qb] = m;
        ls[qb] = 0.f;
    }
    f32x4 o[4][NQB];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) o[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        bf16x8 va[4];
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const unsigned char* vrow = sVt + (db * 16 + l15) * VT_STRIDE + (kt * 32 + 4 * l4) * 2;
            const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow);
            const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vrow + 32);
            va[db][0] = lo[0]; va[db][1] = lo[1]; va[db][2] = lo[2]; va[db][3] = lo[3];
            va[db][4] = hi[0]; va[db][5] = hi[1]; va[db][6] = hi[2]; va[db][7] = hi[3];
        }
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            bf16x8 pb;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ex = __builtin_amdgcn_exp2f(sc[kt][qb][kb][e] - mx[qb]);
                    sc[kt][qb][kb][e] = ex;
                    ls[qb] += ex;
                    pb[4 * kb + e] = (bf16)ex;
                }
            if (drop_on)        // the context uses the masked weights, the row sum the unmasked ones
                pb = attn_drop8_rt(pb, dbase[qb], kt, drop_key, drop_thr2);
            if (side_post) {    // side outputs after the dropout: the scores kept for them take the mask (x 1 / (1 - p) below)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t w = attn_drop_word(dbase[qb], 4 * kt + i, drop_key);
#pragma unroll
                    for (int f = 0; f < 2; ++f)
                        if ((int)(short)(w >> (16 * f)) < thr_s) sc[kt][qb][i >> 1][2 * (i & 1) + f] = 0.f;
                }
            }
#pragma unroll
            for (int db = 0; db < 4; ++db)
                o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[db], pb, o[db][qb], 0, 0, 0);
        }
    }
    float inv_ctx[NQB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        float l = ls[qb];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        inv[qb] = 1.0f / l;
        inv_ctx[qb] = drop_on ? inv[qb] * drop_keep : inv[qb];
        if (side_post) inv[qb] = inv_ctx[qb];               // (inv is used by the side outputs only from here on)
        if (lse_out) {                                      // log2 sum_j exp2(score_ij) = row max + log2 l
            const int qi = qbase + qb * 16 + l15 - P;
            if (l4 == 0 && qi >= 0 && qi < S) lse_out[((int64_t)n * A + a) * S + qi] = mx[qb] + __builtin_amdgcn_logf(l);
        }
    }
    // ---- side outputs: full probabilities (parity tests); head-summed text -> region block --------------
    if (probs) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) {
                const int qi = qbase + qb * 16 + l15 - P;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = kt * 32 + kb * 16 + 4 * l4 + e;
                        if (qi >= 0 && qi < S && key < L)
                            probs[(((int64_t)n * A + a) * S + qi) * L + key] = sc[kt][qb][kb][e] * inv[qb];
                    }
            }
    }
    if (align_map) {
        // both heads add their normalised text->region block into one LDS tile [T][R] (over the V^T images, dead
        // once every wave is past its P.V), then whole rows go out as atomics
        // (one head per workgroup: the tile starts at the K image, which is dead as well -- K | V^T together hold any [T][R] with
        // T + R <= 256; the context transposes below go through the Q image)
        const int T = align_t, R = S - T;
        static_assert(NH == 2 || LP * 128 + 64 * VT_STRIDE >= (LP / 2) * (LP / 2) * 4, "align tile over K | V^T");
        float* sAm = reinterpret_cast<float*>(NH == 1 ? A4::img_qk(smem, 1, 0) : A4::img_vt(smem, 0));
        __syncthreads();
        for (int j = tid; j < T * R; j += A4::NT) sAm[j] = 0.f;
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
            if (kt * 32 + 31 >= T) {
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) {
                    const int qi = qbase + qb * 16 + l15;
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int key = kt * 32 + kb * 16 + 4 * l4 + e;
                            if (qi < T && key >= T && key < L)
                                atomicAdd(sAm + qi * R + (key - T), sc[kt][qb][kb][e] * inv[qb]);
                        }
                }
            }
        __syncthreads();
        float* dst = align_map + (int64_t)n * T * R;
        for (int j = tid; j < T * R; j += A4::NT) atomicAdd(dst + j, sAm[j]);
    }
    attn4_store_ctx<A4>(o, inv_ctx, smem + (hd * LP + qbase) * 128, ctx + (crow + qbase - P) * H + a * 64, H, P - qbase, Ln - qbase, l15, l4, lane);
}

// MODE 0 = generic (probabilities / align map / chunk-mean queries / either mask form, exact row max), one tile
// per workgroup.  Production variants (persistent over tiles): 1 = broadcast key mask, 2 = dense mask bits,
// 3 = dense mask bits + chunk-mean queries + head-summed text->region map (seq_enc layers 9-11): streaming
// softmax without a max pass, row sums checked and the tile redone exactly when one leaves [1e-30, 1e30].
// DUMPV = 1 (two heads per workgroup, streaming variants, p.dump set): the Q | K | V image dump of a trainable layer's forward is
// issued in 18 (12 at LP = 128) pieces per thread BETWEEN the key tiles of phase B instead of as a block in front of it: the dump is
// store-issue work (144 KB per tile), phase B is VALU / MFMA work, and the block cost +58-75 us per call.
// (FOLD, the LayerNorm-fold prototype of DESIGN section 7, is a sixth template parameter in the TUNING build only: the product's
// kernels keep the five-parameter names and the binaries that the profiles/ and PMC files of the round were taken on)
#ifdef MODCR_TUNING
#define A4_FOLD_PARAM , int FOLD = 0
#define A4_FOLD_ARG , FOLD
#else
#define A4_FOLD_PARAM
#define A4_FOLD_ARG
#endif
template <int KMODE, int LP, int DROP, int NHD = 2, int DUMPV = 0 A4_FOLD_PARAM>
__global__ __launch_bounds__(512, 2) void qkv_attn4_kernel(AttnArgs p) {
#ifndef MODCR_TUNING
    constexpr int FOLD = 0;
#endif
    static_assert(!DUMPV || (NHD == 2 && KMODE != 0), "interleaved dump: streaming variants with two heads per workgroup");
    typedef A4T<LP, NHD> A4;
    constexpr int NI = A4::NI, QW = A4::QW, NQB = A4::NQB, NKT = A4::NKT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HA = A4::HA, HB = A4::HB, KT = A4::KT, VT_STRIDE = A4::VT_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / A4::WC, wc = wave % A4::WC;
    const int l15 = lane & 15, l4 = lane >> 4;
    // tuning build, A/B only: static priority for one half of the waves for the whole kernel (MI355X_MICROARCH.md "Two waves per SIMD"
    // item 4); debug bit 8 raises waves 4-7 (the younger half), bit 9 waves 0-3 (the control)
    if (MODCR_DBG(p.debug & 256) && wave >= 4) __builtin_amdgcn_s_setprio(1);
    if (MODCR_DBG(p.debug & 512) && wave < 4) __builtin_amdgcn_s_setprio(1);
    float* sMask = reinterpret_cast<float*>(smem + A4::MAIN);
    float* sBias = sMask + LP;                              // [head][q|k|v][64]
    int* sCid = reinterpret_cast<int*>(sBias + A4::NF);
    int* sFlag = sCid + LP;                                 // [0] redo the tile with the exact pass, [1] chunks are not contiguous runs
    int* sFirst = sFlag + 4;                                // per chunk id: first / last token, token count
    int* sLast = sFirst + LP;
    int* sCnt = sLast + LP;

    const int hgroups = p.A / NHD;
    const int ntiles = p.N * hgroups;
    // prefix rows (history_state, modeling_bert.py:36-44): p.x then holds [prefix ; x] rows per sequence (the host entry
    // concatenates them), tile rows / keys 0..L-1 with L = P + S, query rows = tile rows P..L-1 -> output rows 0..S-1
    const int S = p.S, P = p.P, L = p.S + p.P, H = p.H;
    int n = 0, a0 = 0;                                      // sequence and first head of the current tile
    int Ln = L;                                             // tile rows of sequence n that exist: L, or its live rows (p.row_start)
    int64_t crow = 0;                                       // first row of sequence n in x (P = 0) and ctx: n * S, or row_start[n]

    // ---- DMA sources: uniform base (sequence / weight matrix + k offset) + 32-bit per-lane byte offset.
    // A half mh: LDS row r (0..95) = token (r / 48) * 96 + mh * 48 + r % 48; piece `wave` (8 rows) by all
    // 64 lanes, rows 64 + 4 wave.. by lanes 0..31 (the LDS address of an LDS-DMA is base + 16 lane).
    // B half nh: LDS row r (0..191) = wave column r / 48, feature slot cc = r % 48 of that column.
    unsigned offA[2][2], vB;
    // B pieces hold 8 consecutive weight rows (a piece never straddles a 16-feature block), so the source is
    // a per-piece scalar row (wbrow, relative to head a0's rows) + ONE per-lane offset: row (lane / 8) and the
    // swizzled chunk, whose key (r >> 1) & 7 = (4 piece + lane / 16) & 7 depends on the piece's parity = wave & 1.
    // (NH = 1: a B half is 96 rows = one piece per wave + half a piece: rows 64 + 4 wave.. by lanes 0..31 with their own
    // per-lane offset vB2, whose swizzle key (r >> 1) & 7 = (2 wave + lane / 16) & 7 depends on wave & 3)
    int wbrow[2][3];
    unsigned vB2 = 0;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int q = 0; q < A4::NBI; ++q) {
            const int r = (NHD == 1 && q == 1) ? 64 + 4 * wave : 8 * (wave + 8 * q);
            const int wcr = r / 48, cc = r % 48;
            int part, d;
            if (nh == 0) { part = wcr & 1; d = cc; }
            else if (cc < 16) { part = wcr & 1; d = 48 + cc; }
            else { part = 2; d = (wcr & 1) * 32 + cc - 16; }
            wbrow[nh][q] = part * H + (wcr >> 1) * 64 + d;
        }
    auto uniform_ptr = [](const void* q) {
        const uint64_t b64 = reinterpret_cast<uint64_t>(q);
        return reinterpret_cast<const char*>(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(b64 >> 32)) << 32) |
                                             (unsigned)__builtin_amdgcn_readfirstlane((int)(b64 & 0xffffffffu)));
    };
    const bf16* xb = p.x;                                   // x of sequence n / Wqkv from head a0's rows on (per tile)
    const bf16* wt = p.wqkv;
    // kind: 0 = A0, 1 = B0, 2 = B1, 3 = A1 (staging order); LDS order inside a K-tile buffer: A0 A1 B0 B1
    auto stage_half = [&](int buf, int kind, int k0) {
        if (kind == 0 || kind == 3) {
            const int mh = kind == 3;
            unsigned char* dst = smem + buf * KT + mh * HA;
            const char* base = uniform_ptr(xb + k0);
            glds16(offA[mh][0], base, dst + wave * 1024);
            if constexpr (A4::NA == 2 && A4::A_HALF_PIECE) { if (lane < 32) glds16(offA[mh][1], base, dst + 8192 + wave * 512); }
            if constexpr (A4::NA == 2 && !A4::A_HALF_PIECE) glds16(offA[mh][1], base, dst + 8192 + wave * 1024);
        } else {
            const int nh = kind == 2;
            unsigned char* dst = smem + buf * KT + 2 * HA + nh * HB;
            if constexpr (NHD == 2) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    glds16(vB, uniform_ptr(wt + (int64_t)wbrow[nh][q] * H + k0), dst + (wave + 8 * q) * 1024);
            } else {
                glds16(vB, uniform_ptr(wt + (int64_t)wbrow[nh][0] * H + k0), dst + wave * 1024);
                if (lane < 32) glds16(vB2, uniform_ptr(wt + (int64_t)wbrow[nh][1] * H + k0), dst + 8192 + wave * 512);
            }
        }
    };

    typedef const __attribute__((address_space(3))) bf16x8* lds_v8;
    unsigned aA[2][2], aB[2][2];

    f32x4 acc[2][2][NI][3];
    bf16x8 fa[NI][2], fb[2][3][2];
    auto rdA = [&](int buf, int mh) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            fa[i][0] = *(lds_v8)(aA[buf][0] + mh * HA + i * 2048);
            fa[i][1] = *(lds_v8)(aA[buf][1] + mh * HA + i * 2048);
        }
    };
    auto rdB = [&](int buf, int nh) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            fb[nh][j][0] = *(lds_v8)(aB[buf][0] + nh * HB + j * 2048);
            fb[nh][j][1] = *(lds_v8)(aB[buf][1] + nh * HB + j * 2048);
        }
    };
    const int nk = MODCR_DBG(p.debug & 2) ? 4 : (H >> 6);       // K-tiles (even, >= 4); debug bit 1: timing-only short loop
    // (128-token tile only: the other tiles' K loops are compiled as before)
    constexpr bool SKIP_PAD = (LP == 128);
    [[maybe_unused]] const bool skip_last = SKIP_PAD && (wr * A4::RW + QW + (NI - 1) * 16 >= p.S + p.P) && !MODCR_DBG(p.debug & 4096);
    // phase I of an 8-phase trip (two K-tiles).  KMODE 0 = steady state, 1 = last trip.
    auto phase = [&](auto I_, auto MODE_, int kt) {
        constexpr int I = decltype(I_)::value, MODE = decltype(MODE_)::value;
        constexpr int Q = I & 3, BUF = I >> 2;
        constexpr int MH = (Q >= 2), NH = (Q == 1 || Q == 2);
        if constexpr (Q == 0) { rdB(BUF, 0); __builtin_amdgcn_sched_barrier(0); rdA(BUF, 0); }
        if constexpr (Q == 1) rdB(BUF, 1);
        if constexpr (Q == 2) rdA(BUF, 1);
        if constexpr (MODE != 1 || I < 2) {
            constexpr int KIND = (I + 2) & 3, DT = (I + 6) >> 2;
            stage_half(DT & 1, KIND, (kt + DT) << 6);
        }
        // DMA instructions per wave that may stay in flight: the last min(4, remaining) half-tiles staged
        constexpr int VM = MODE != 1 ? A4::FLY4 : (I <= 1 ? A4::FLY4 : I == 2 ? A4::NA + 2 * A4::NBI : I == 3 ? A4::NA + A4::NBI : I == 4 ? A4::NA : 0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_setprio(1);
        auto block = [&](int ks, int i, int j) {
            if (NH == 1 && j >= 1)   // v: tokens in registers, features on lanes
                acc[MH][NH][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][ks], fb[NH][j][ks], acc[MH][NH][i][j], 0, 0, 0);
            else                     // q, k: features in registers, tokens on lanes
                acc[MH][NH][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[NH][j][ks], fa[i][ks], acc[MH][NH][i][j], 0, 0, 0);
        };
        if constexpr (SKIP_PAD && MH == 1) {
            // 128-token tile (round 6): the last 16-token block of a wave row's second half (tokens 112..127 for wave row 1) is pure tile
            // padding whenever L <= 112 -- the image-only pass (S = 101) and the RoBERTa body (P + S = 111) -- and its products are the
            // only difference to a 112-token tile in this phase: skipped (its accumulators stay 0; those image rows are masked keys and
            // unstored queries).  One wave of every SIMD is a wave-row-1 wave, so the MH = 1 phases drop from 24 to 18 MFMAs per SIMD.
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < NI - 1; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) block(ks, i, j);
            if (!skip_last) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int j = 0; j < 3; ++j) block(ks, NI - 1, j);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) block(ks, i, j);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    auto trip = [&](auto MODE_, int kt) {
        phase(std::integral_constant<int, 0>{}, MODE_, kt);
        phase(std::integral_constant<int, 1>{}, MODE_, kt);
        phase(std::integral_constant<int, 2>{}, MODE_, kt);
        phase(std::integral_constant<int, 3>{}, MODE_, kt);
        phase(std::integral_constant<int, 4>{}, MODE_, kt);
        phase(std::integral_constant<int, 5>{}, MODE_, kt);
        phase(std::integral_constant<int, 6>{}, MODE_, kt);
        phase(std::integral_constant<int, 7>{}, MODE_, kt);
    };
    // Persistent: workgroup b walks tiles b, b + gridDim, ... (gridDim is a multiple of 8, so a workgroup's
    // tiles stay in its XCD's chunk of the tile order); no workgroup launch / LDS hand-over between tiles.
    // (A sequence-major walk -- one workgroup owns a sequence's six head pairs, its align map accumulated by plain
    // read-add-write -- measured 178 vs 174 us at N = 256 and 269 vs 257 us for MODE 3: not kept.)
    [[maybe_unused]] int trace_it = 0;
    [[maybe_unused]] auto trace = [&](int ev) {
        if (MODCR_DBG(p.trace != nullptr)) {
            if (blockIdx.x == 0 && lane == 0 && (wave & 3) == 0 && trace_it < 32) p.trace[(wave >> 2) * 512 + trace_it * 8 + ev] = __builtin_readcyclecounter();
        }
    };
    for (int vt = blockIdx.x; vt < ntiles; vt += gridDim.x) {
    trace(0);
    {
        if (p.hconc > 0 && (p.N & 7) == 0) {
            // head-pair-major inside an XCD, `hconc` head pairs at a time: the workgroups resident on an XCD share hconc weight
            // slices (hconc x 590 KB of its 4 MB L2) instead of all of Wqkv
            const int xcd = vt & 7, idx = vt >> 3, ns = p.N >> 3, G = p.hconc;
            const int hgb = idx / (ns * G), rem = idx - hgb * ns * G;
            const int gw = min(G, hgroups - hgb * G);
            n = xcd * ns + rem / gw;
            a0 = (hgb * G + rem % gw) * NHD;
        } else {
            const int tile = xcd_remap(vt, ntiles);
            n = tile / hgroups; a0 = (tile % hgroups) * NHD;
        }
        if (p.row_start) {
            // (clamped to the buffer's N * S rows: a table that is not what the host builder makes cannot send an access out of it)
            Ln = min(max(p.row_start[n + 1] - p.row_start[n], 1), L);
            crow = min(max(p.row_start[n], 0), p.N * L - Ln);
            xb = p.x + crow * H;
        } else {
            Ln = L;
            crow = (int64_t)n * S;
            xb = p.x + (int64_t)n * L * H;
        }
        wt = p.wqkv + (int64_t)a0 * 64 * H;
    }
    {
        // Per-tile recomputation (from an opaque copy of the thread id) of every per-lane address the K loop
        // needs: kept loop-invariant across tiles they would stay live through phase B and spill there.
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int lane = tq & 63, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
        for (int mh = 0; mh < 2; ++mh)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r = q == 0 ? 8 * wave + (lane >> 3)
                                     : (A4::A_HALF_PIECE ? 64 + 4 * wave + ((lane & 31) >> 3) : 64 + 8 * wave + (lane >> 3));
                const int tok = min((r / QW) * A4::RW + mh * QW + (r % QW), Ln - 1);     // padding rows re-read the last row
                const int c = (lane & 7) ^ ((r >> 1) & 7);
                offA[mh][q] = (unsigned)((tok * H + c * 8) * 2);
            }
        vB = (unsigned)((((lane >> 3) * H) + (((lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7)) * 8)) * 2);
        if constexpr (NHD == 1) vB2 = (unsigned)(((((lane & 31) >> 3) * H) + (((lane & 7) ^ ((2 * wave + ((lane & 31) >> 4)) & 7)) * 8)) * 2);
    const int keyr = (l15 >> 1) & 7;
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
        const unsigned ck0 = ((l4 ^ keyr) & 7) << 4, ck1 = (((l4 + 4) ^ keyr) & 7) << 4;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            aA[b][0] = lds0 + b * KT + (wr * QW + l15) * 128 + ck0;
            aA[b][1] = lds0 + b * KT + (wr * QW + l15) * 128 + ck1;
            aB[b][0] = lds0 + b * KT + 2 * HA + (wc * 48 + l15) * 128 + ck0;
            aB[b][1] = lds0 + b * KT + 2 * HA + (wc * 48 + l15) * 128 + ck1;
            asm volatile("" : "+v"(aA[b][0]), "+v"(aA[b][1]), "+v"(aB[b][0]), "+v"(aB[b][1]));
        }

    }
    {
        int tidb = tid;                                     // opaque per tile: keeps this address math inside the loop
        asm volatile("" : "+v"(tidb));
        if (tidb < LP) {
            const int j = tidb;
            float m;
            if (j >= L) m = -INFINITY;
            else if (p.bits) m = 0.f;
            else m = (1.0f - p.key_mask[(int64_t)n * L + j]) * (MODCR_NEG * LOG2E);
            sMask[j] = m;
            sCid[j] = (p.chunk_id && j < p.chunk_t) ? p.chunk_id[(int64_t)n * p.chunk_t + j] : -1;
        }
        if (tidb == 0) {
            sFlag[0] = 0; sFlag[1] = 0;
            uint32_t* sDrop = reinterpret_cast<uint32_t*>(smem + A4::DROP_OFF);      // read by attn4_exact_tail
            sDrop[0] = p.drop_thr2; sDrop[1] = (uint32_t)p.drop_key; sDrop[2] = (uint32_t)(p.drop_key >> 32);
            sDrop[3] = __float_as_uint(((KMODE == 0 || DROP) && p.drop_on) ? p.drop_keep : 1.0f);
            sDrop[4] = (uint32_t)P;
            const uint64_t lp64 = reinterpret_cast<uint64_t>(p.lse);
            sDrop[5] = (uint32_t)lp64; sDrop[6] = (uint32_t)(lp64 >> 32);
            sDrop[7] = (uint32_t)p.side_post_drop;
            sDrop[8] = (uint32_t)crow; sDrop[9] = (uint32_t)((uint64_t)crow >> 32); sDrop[10] = (uint32_t)Ln;
        }
        if (((KMODE == 0 && p.chunk_id) || KMODE == 3) && tidb < LP) { sFirst[tidb] = LP; sLast[tidb] = -1; sCnt[tidb] = 0; }
        if (tidb < A4::NF) {
            const int j = tidb, jh = j / 192, jj = j % 192;
            sBias[j] = p.bqkv[(jj >> 6) * H + (a0 + jh) * 64 + (jj & 63)];
#ifdef MODCR_TUNING
            if constexpr (FOLD) reinterpret_cast<float*>(smem + A4::FOLD_OFF)[2 * LP + j] = p.cfold[(jj >> 6) * H + (a0 + jh) * 64 + (jj & 63)];
#endif
        }
#ifdef MODCR_TUNING
        if constexpr (FOLD) {
            if (tidb < LP) {
                float* sRs = reinterpret_cast<float*>(smem + A4::FOLD_OFF);
                const float2 st = tidb < L ? *reinterpret_cast<const float2*>(p.row_stats + ((int64_t)n * L + tidb) * 2) : float2{0.f, 0.f};
                sRs[tidb] = st.x; sRs[LP + tidb] = st.y;
            }
        }
#endif
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // half-tiles 0..5 = A0 B0 B1 A1 of K-tile 0, A0 B0 of K-tile 1
    stage_half(0, 0, 0); stage_half(0, 1, 0); stage_half(0, 2, 0); stage_half(0, 3, 0);
    stage_half(1, 0, 64); stage_half(1, 1, 64);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A4::FLY4) : "memory");      // A0, B0 of K-tile 0 landed
    __builtin_amdgcn_s_barrier();
    if ((wave >> 2) == 1) __builtin_amdgcn_s_barrier();     // group 1 (waves 4..7: one of each group per SIMD) runs one barrier behind
    __builtin_amdgcn_sched_barrier(0);
    trace(1);
    for (int kt = 0; kt + 2 < nk; kt += 2) trip(std::integral_constant<int, 0>{}, kt);
    trip(std::integral_constant<int, 1>{}, nk - 2);
    if ((wave >> 2) == 0) __builtin_amdgcn_s_barrier();     // realign: every wave is done with the ring
    __builtin_amdgcn_sched_barrier(0);
    trace(2);
    // Per-tile copies of the lane indices the compiler cannot see through: everything below is loop-invariant
    // address arithmetic, and hoisted out of the tile loop it would pin > 100 registers across the K loop.
    int l15b = l15, l4b = l4, laneb = lane;
    asm volatile("" : "+v"(l15b), "+v"(l4b), "+v"(laneb));
    [[maybe_unused]] const int tid_d = wave * 64 + laneb;                // (per-tile opaque: the interleaved dump's addresses)

    // dense mask words of this wave's phase-B queries, issued now so they land under the image pass
    uint32_t wd[NQB][NKT];
    auto load_mask_words = [&]() {
        const int LWp = (L + 31) >> 5;
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            const int qi = (wave % A4::WPH) * QW + qb * 16 + l15b - P;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
                wd[qb][kt] = (qi >= 0 && qi < S && kt < LWp) ? p.bits[((int64_t)n * S + qi) * LWp + kt] : 0xffffffffu;
        }
    };
    if constexpr (KMODE == 2) load_mask_words();
    // ---- Q (scaled by log2(e)/8), K, V^T (+bias) as bf16 images: [Q0 | Q1 | K0 | K1 | Vt0 | Vt1] ------------
    const int hd_a = wc >> 1, part_a = wc & 1;              // this wave's q/k part and head in phase A
    {
        unsigned char* sQK = A4::img_qk(smem, part_a, hd_a);
        unsigned char* sVt = A4::img_vt(smem, hd_a);
        const float* bqk = sBias + hd_a * 192 + part_a * 64;
        const float* bv = sBias + hd_a * 192 + 128;
        const float qs = part_a == 0 ? 0.125f * LOG2E : 1.0f;
#pragma unroll
        for (int mh = 0; mh < 2; ++mh)
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int tb = wr * A4::RW + mh * QW + i * 16;
                [[maybe_unused]] const float* sRs = reinterpret_cast<const float*>(smem + A4::FOLD_OFF);
                [[maybe_unused]] const float* sCf = sRs + 2 * LP + hd_a * 192;
                [[maybe_unused]] float rs_t = 1.f, rm_t = 0.f;          // FOLD: rstd and rstd * mu of this lane's q / k token
                if constexpr (FOLD) { rs_t = sRs[tb + l15b]; rm_t = sRs[LP + tb + l15b]; }
#pragma unroll
                for (int b = 0; b < 4; ++b) {               // q/k feature blocks: d0 = 16 b
                    const f32x4& v = acc[mh][b == 3][i][b == 3 ? 0 : b];
                    const int d0 = 16 * b + 4 * l4b;
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(bqk + d0);
                    bf16x4 o;
                    if constexpr (FOLD) {                   // LayerNorm folded into the projection: rstd acc - rstd mu c + d
                        const f32x4 cf = *reinterpret_cast<const f32x4*>(sCf + part_a * 64 + d0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (bf16)((fmaf(v[e], rs_t, bs[e]) - rm_t * cf[e]) * qs);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (bf16)((v[e] + bs[e]) * qs);
                    }
                    *reinterpret_cast<bf16x4*>(sQK + swz128(tb + l15b, d0 >> 3) + (d0 & 7) * 2) = o;
                }
#pragma unroll
                for (int j = 1; j < 3; ++j) {               // v feature blocks
                    const int d = part_a * 32 + (j - 1) * 16 + l15b;
                    const float bb = bv[d];
                    const f32x4& v = acc[mh][1][i][j];
                    bf16x4 o;
                    if constexpr (FOLD) {                   // four tokens of one feature per lane
                        const f32x4 r4 = *reinterpret_cast<const f32x4*>(sRs + tb + 4 * l4b), m4 = *reinterpret_cast<const f32x4*>(sRs + LP + tb + 4 * l4b);
                        const float cv = sCf[128 + d];
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (bf16)(fmaf(v[e], r4[e], bb) - m4[e] * cv);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (bf16)(v[e] + bb);
                    }
                    *reinterpret_cast<bf16x4*>(sVt + d * VT_STRIDE + (tb + 4 * l4b) * 2) = o;
                }
            }
    }
    __syncthreads();
    trace(3);

    const int hd = wave / A4::WPH, qbase = (wave % A4::WPH) * QW;      // phase B: head, first query
    unsigned char* sQ = A4::img_qk(smem, 0, hd);
    unsigned char* sK = A4::img_qk(smem, 1, hd);
    unsigned char* sVt = A4::img_vt(smem, hd);
    const int a = a0 + hd;

    // ---- chunk-mean query (phase-3 layers of seq_enc, v10:66-78): out of line, see attn4_chunk_mean ---------
    if constexpr (KMODE == 0 || KMODE == 3) {
        if ((KMODE == 3 || p.chunk_id) && !MODCR_DBG(p.debug & 16))        // debug bit 4: timing-only, no chunk means
            attn4_chunk_mean<LP, NHD>(smem, p.chunk_t, tid);
    }
    if (MODCR_DBG(p.debug & 1)) { __syncthreads(); continue; }
    // ---- training forward of a layer that will be differentiated: the images leave as rows (Q scaled by log2e / 8 and
    // chunk-averaged exactly as phase B sees it; V transposed back by ds_read_b64_tr_b16), 72 KB per head at LP = 192
    if constexpr (NHD == 2 && !DUMPV) {
        if (p.dump) {
            int td = tid;
            asm volatile("" : "+v"(td));
            typedef __attribute__((address_space(3))) bf16x4* lds_tr;
#pragma unroll 1
            for (int hh = 0; hh < 2; ++hh) {
                bf16* dst = p.dump + ((int64_t)n * p.A + a0 + hh) * (3 * LP * 64);
                const unsigned char* iq = A4::img_qk(smem, 0, hh);
                const unsigned char* ik = A4::img_qk(smem, 1, hh);
                const unsigned char* iv = A4::img_vt(smem, hh);
#pragma unroll 1
                for (int it = td; it < LP * 8; it += A4::NT) {
                    const int r = it >> 3, c = it & 7;
                    *reinterpret_cast<uint4*>(dst + r * 64 + c * 8) = *reinterpret_cast<const uint4*>(iq + swz128(r, c));
                    *reinterpret_cast<uint4*>(dst + LP * 64 + r * 64 + c * 8) = *reinterpret_cast<const uint4*>(ik + swz128(r, c));
                }
                // V rows: a 16-lane group reads the 4 x 16 block (features 8 c .. + 3 | + 4 .. + 7, keys 16 kb ..) of the V^T image
                // transposed: lane i receives key 16 kb + i, eight consecutive features = one 16-byte piece of its row
#pragma unroll 1
                for (int it = td; it < LP * 8; it += A4::NT) {          // LP * 8 / 512 whole trips: EXEC stays full
                    const int pi = it >> 4, i = it & 15, kb16 = pi >> 3, c = pi & 7;
                    const unsigned char* at = iv + (c * 8 + (i >> 2)) * VT_STRIDE + (kb16 * 16 + (i & 3) * 4) * 2;
                    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr)(at));
                    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr)(at + 4 * VT_STRIDE));
                    bf16x8 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
                    *reinterpret_cast<bf16x8*>(dst + 2 * LP * 64 + (kb16 * 16 + i) * 64 + c * 8) = v;
                }
            }
        }
    }
    if constexpr (KMODE == 3) load_mask_words();            // after the call above (18 registers it would have to save)

    // ---- phase B ----------------------------------------------------------------------------------------
    // S^T block (kt, kb, qb): key = 32 kt + 16 kb + 4 l4b + e in register e, query = qbase + 16 qb + l15b.
    if constexpr (KMODE == 0) {
        attn4_exact_tail<LP, NHD>(smem, p.bits, p.probs, p.align_map, p.ctx, p.align_t, S, H, p.A, n, a0, tid);
        break;                                              // the generic variant is launched one tile per workgroup
    } else {
        // streaming pass: P' = exp2(S) with no row max (scores are log2-domain, masked keys sit at -14427 or
        // -inf and flush to 0), tile kt+1's Q.K^T issued ahead of tile kt's exponentials; the row sum comes
        // out of the matrix pipe as a fifth V^T block of ones (summed over the bf16 P' the numerator uses).
        f32x4 o[4][NQB];
        float inv[NQB];
        bf16x8 fq[NQB][2];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                fq[qb][ks] = *reinterpret_cast<const bf16x8*>(sQ + swz128(qbase + qb * 16 + l15b, ks * 4 + l4b));
        bf16x8 ones;
#pragma unroll
        for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.0f;
        [[maybe_unused]] uint32_t dbase[NQB];               // dropout bases of this lane's query rows and key group l4b (attn_common.h)
        [[maybe_unused]] uint64_t dkey = p.drop_key;        // kept in a register pair: the addend of every v_mad_u64_u32 below
        if constexpr (DROP) {
            asm volatile("" : "+v"(dkey));
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) dbase[qb] = attn_drop_base((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + qbase + qb * 16 + l15b - P), (uint32_t)l4b, dkey);
        }
        f32x4 ol[NQB];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            ol[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        auto qk_block = [&](int kt, int kb, int qb, const bf16x8& fk0, const bf16x8& fk1, const f32x4& mk) {
            f32x4 c = mk;
            if constexpr (KMODE == 2 || KMODE == 3) {       // dense mask: bit (16 kb + 4 l4b + e) of this query's word
                const uint32_t w2 = wd[qb][kt] >> (4 * l4b);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (!((w2 >> (kb * 16 + e)) & 1u)) c[e] += MODCR_NEG * LOG2E;
            }
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk0, fq[qb][0], c, 0, 0, 0);
            return __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk1, fq[qb][1], c, 0, 0, 0);
        };
        auto qk_tile = [&](auto KT_, f32x4 (&s)[NQB][2]) {
            constexpr int kt = decltype(KT_)::value;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int krow = kt * 32 + kb * 16;
                const bf16x8 fk0 = *reinterpret_cast<const bf16x8*>(sK + swz128(krow + l15b, l4b));
                const bf16x8 fk1 = *reinterpret_cast<const bf16x8*>(sK + swz128(krow + l15b, 4 + l4b));
                const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + krow + 4 * l4b);
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) s[qb][kb] = qk_block(kt, kb, qb, fk0, fk1, mk);
            }
        };
        auto pv_tile = [&](auto KT_, const f32x4 (&s)[NQB][2]) {
            constexpr int kt = decltype(KT_)::value;
            // (round 6, measured and removed: alternating s_setprio between the two wave halves key tile by key tile, so that the younger
            // wave of a SIMD -- which finishes this VALU-bound phase alone, 13.2 k against 8.1 k cycles -- is not left with a solo tail:
            // 378.7 -> 377.8 us per tile, every second tile 381.5; profiles/r06_ab_attn_skip_and_alternate.log)
            bf16x8 va[4];
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const unsigned char* vrow = sVt + (db * 16 + l15b) * VT_STRIDE + (kt * 32 + 4 * l4b) * 2;
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow);
                const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vrow + 32);
                va[db][0] = lo[0]; va[db][1] = lo[1]; va[db][2] = lo[2]; va[db][3] = lo[3];
                va[db][4] = hi[0]; va[db][5] = hi[1]; va[db][6] = hi[2]; va[db][7] = hi[3];
            }
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) {
                bf16x8 pb;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) pb[4 * kb + e] = (bf16)__builtin_amdgcn_exp2f(s[qb][kb][e]);
                ol[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pb, ol[qb], 0, 0, 0);     // row sum: unmasked weights
                if constexpr (DROP) pb = attn_drop8<kt>(pb, dbase[qb], dkey, p.drop_thr2);
#pragma unroll
                for (int db = 0; db < 4; ++db)
                    o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[db], pb, o[db][qb], 0, 0, 0);
            }
        };
        // interleaved dump (DUMPV): piece q of this thread = (head, Q | K | V, item td + 512 itn), three pieces per key tile
        [[maybe_unused]] auto dump_slot = [&](auto SLOT_) {
            if constexpr (DUMPV) {
                constexpr int slot = decltype(SLOT_)::value;
                constexpr int IT = LP * 8 / A4::NT;                     // items per thread, head and image (3 / 2)
                static_assert(2 * 3 * IT == 3 * NKT, "three dump pieces per key tile");
                typedef __attribute__((address_space(3))) bf16x4* lds_tr;
#pragma unroll
                for (int q = 3 * slot; q < 3 * slot + 3; ++q) {
                    const int hh = q / (3 * IT), kind = (q % (3 * IT)) / IT, it = tid_d + (q % IT) * A4::NT;
                    bf16* dst = p.dump + ((int64_t)n * p.A + a0 + hh) * (3 * LP * 64);
                    if (kind < 2) {
                        const int r = it >> 3, c = it & 7;
                        const unsigned char* img = A4::img_qk(smem, kind, hh);
                        *reinterpret_cast<uint4*>(dst + kind * LP * 64 + r * 64 + c * 8) = *reinterpret_cast<const uint4*>(img + swz128(r, c));
                    } else {
                        // V rows: a 16-lane group reads the 4 x 16 block of the V^T image transposed (see the block form above)
                        const unsigned char* iv = A4::img_vt(smem, hh);
                        const int pi = it >> 4, i = it & 15, kb16 = pi >> 3, c = pi & 7;
                        const unsigned char* at = iv + (c * 8 + (i >> 2)) * VT_STRIDE + (kb16 * 16 + (i & 3) * 4) * 2;
                        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr)(at));
                        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_tr)(at + 4 * VT_STRIDE));
                        bf16x8 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
                        *reinterpret_cast<bf16x8*>(dst + 2 * LP * 64 + (kb16 * 16 + i) * 64 + c * 8) = v;
                    }
                }
            }
        };
        {
            f32x4 sA[NQB][2], sB[NQB][2];
            qk_tile(std::integral_constant<int, 0>{}, sA);
            qk_tile(std::integral_constant<int, 1>{}, sB); dump_slot(std::integral_constant<int, 0>{}); pv_tile(std::integral_constant<int, 0>{}, sA);
            qk_tile(std::integral_constant<int, 2>{}, sA); dump_slot(std::integral_constant<int, 1>{}); pv_tile(std::integral_constant<int, 1>{}, sB);
            qk_tile(std::integral_constant<int, 3>{}, sB); dump_slot(std::integral_constant<int, 2>{}); pv_tile(std::integral_constant<int, 2>{}, sA);
            if constexpr (NKT == 8) {
                qk_tile(std::integral_constant<int, 4>{}, sA); pv_tile(std::integral_constant<int, 3>{}, sB);
                qk_tile(std::integral_constant<int, 5>{}, sB); pv_tile(std::integral_constant<int, 4>{}, sA);
                qk_tile(std::integral_constant<int, 6>{}, sA); pv_tile(std::integral_constant<int, 5>{}, sB);
                qk_tile(std::integral_constant<int, 7>{}, sB); pv_tile(std::integral_constant<int, 6>{}, sA);
                pv_tile(std::integral_constant<int, 7>{}, sB);
            } else if constexpr (NKT == 6) {
                qk_tile(std::integral_constant<int, 4>{}, sA); dump_slot(std::integral_constant<int, 3>{}); pv_tile(std::integral_constant<int, 3>{}, sB);
                qk_tile(std::integral_constant<int, 5>{}, sB); dump_slot(std::integral_constant<int, 4>{}); pv_tile(std::integral_constant<int, 4>{}, sA);
                dump_slot(std::integral_constant<int, 5>{}); pv_tile(std::integral_constant<int, 5>{}, sB);
            } else {
                dump_slot(std::integral_constant<int, 3>{}); pv_tile(std::integral_constant<int, 3>{}, sB);
            }
        }
        bool ok = true;
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            const float l = ol[qb][0];                      // every register of the ones block holds the row sum
            ok = ok && (l > 1e-30f) && (l < 1e30f);
            inv[qb] = 1.0f / l;
        }

        // a row sum out of range anywhere in the workgroup -> everybody redoes the tile with the exact pass
        if ((!__all(ok) || MODCR_DBG(p.debug & 8)) && laneb == 0) *sFlag = 1;
        trace(4);
        __syncthreads();
        trace(5);
        // The exact pass is called AFTER the common path's block, from its own re-read of the flag: inside an if / else
        // with the call in one arm, the compiler parks the accumulators in scratch ahead of the branch on every tile
        // (measured: 100 MB of scratch writes per launch).
        if (!*sFlag) {
            if (p.lse) {                                    // row statistics for the backward: log2 of the (unmasked) row sum
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) {
                    const int qi = qbase + qb * 16 + l15b - P;
                    if (l4b == 0 && qi >= 0 && qi < S) p.lse[((int64_t)n * p.A + a) * S + qi] = -__builtin_amdgcn_logf(inv[qb]);
                }
            }
            // context rows first (Q frags are in registers: the wave's own Q rows are free for the transpose), so that
            // the accumulators are dead during the align-map pass
            if constexpr (DROP) {                           // the context rows carry dropout's 1 / (1 - p)
                float inv_ctx[NQB];
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) inv_ctx[qb] = inv[qb] * p.drop_keep;
                attn4_store_ctx<A4>(o, inv_ctx, sQ + qbase * 128, p.ctx + (crow + qbase - P) * H + a * 64, H, P - qbase, Ln - qbase, l15b, l4b, laneb);
            } else {
                attn4_store_ctx<A4>(o, inv, sQ + qbase * 128, p.ctx + (crow + qbase - P) * H + a * 64, H, P - qbase, Ln - qbase, l15b, l4b, laneb);
            }
            if (KMODE == 3 && !MODCR_DBG(p.debug & 32)) {                // debug bit 5: timing-only, no align map
                // head-summed text -> region block, no LDS atomics: each head has its OWN [T][R] tile in LDS (head 0 over the
                // V^T images, head 1 over the Q images: both dead once every wave is past the barrier below; K stays, the
                // scores are recomputed from it) and a wave owns its 48 query rows, so the P' / l values go out as plain
                // 16-byte stores straight from the recomputed score blocks.  The sum of the two tiles then goes to the [N,T,R]
                // map in HBM as float atomics (six head-pair tiles and three layers meet there; fire-and-forget: a
                // read-add-write by an owning workgroup measured slower).
                const int T = p.align_t, R = S - T;
                // (one head per workgroup, LP = 256: its tile over the V^T image; the launcher checks that it fits)
                float* sAm = reinterpret_cast<float*>(hd == 0 ? A4::img_vt(smem, 0) : smem);
                const bool vec = ((T | R) & 3) == 0;            // 16-byte pieces: a lane's four keys are in or out together
                __syncthreads();                                    // every wave is done with Q rows (context transposes) and V^T
                if (qbase < T) {
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt)
                        if (kt * 32 + 31 >= T) {
#pragma unroll
                            for (int kb = 0; kb < 2; ++kb) {
                                const int krow = kt * 32 + kb * 16, key0 = krow + 4 * l4b;
                                const bf16x8 fk0 = *reinterpret_cast<const bf16x8*>(sK + swz128(krow + l15b, l4b));
                                const bf16x8 fk1 = *reinterpret_cast<const bf16x8*>(sK + swz128(krow + l15b, 4 + l4b));
                                const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + krow + 4 * l4b);
#pragma unroll
                                for (int qb = 0; qb < NQB; ++qb) {
                                    const int qi = qbase + qb * 16 + l15b;
                                    const f32x4 sv = qk_block(kt, kb, qb, fk0, fk1, mk);
                                    f32x4 v;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_exp2f(sv[e]) * inv[qb];
                                    if constexpr (DROP) {
                                        if (p.side_post_drop) {         // the map sums the probabilities AFTER the dropout (v10:94-106)
                                            const int thr_s = (int)(short)(p.drop_thr2 & 0xffffu) + 1;
#pragma unroll
                                            for (int i = 0; i < 2; ++i) {
                                                const uint32_t w = attn_drop_word(dbase[qb], (2 * kt + kb) * 2 + i, dkey);
#pragma unroll
                                                for (int f = 0; f < 2; ++f)
                                                    v[2 * i + f] = (int)(short)(w >> (16 * f)) >= thr_s ? v[2 * i + f] * p.drop_keep : 0.f;
                                            }
                                        }
                                    }
                                    if (qi >= T) continue;
                                    float* at = sAm + qi * R + (key0 - T);
                                    if (vec) {
                                        if (key0 >= T && key0 < L) *reinterpret_cast<f32x4*>(at) = v;
                                    } else {
#pragma unroll
                                        for (int e = 0; e < 4; ++e)
                                            if (key0 + e >= T && key0 + e < L) at[e] = v[e];
                                    }
                                }
                            }
                        }
                }
                __syncthreads();
                const float* sA0 = reinterpret_cast<const float*>(A4::img_vt(smem, 0));
                const float* sA1 = reinterpret_cast<const float*>(smem);
                float* dst = p.align_map + (int64_t)n * T * R;
                // (debug bits 6 / 7, timing only: no output at all / plain stores instead of atomics -- what VERDICT r04 item 2b's
                // per-head-pair partial tiles would issue, without their fold: tools/ab_align_atomics.py)
                if (MODCR_DBG(p.debug & 64)) {
                } else if (MODCR_DBG(p.debug & 128)) {
                    for (int j = tid; j < T * R; j += A4::NT) dst[j] = sA0[j] + (NHD == 2 ? sA1[j] : 0.f);
                } else if constexpr (NHD == 2) {
                    for (int j = tid; j < T * R; j += A4::NT) atomicAdd(dst + j, sA0[j] + sA1[j]);
                } else {
                    for (int j = tid; j < T * R; j += A4::NT) atomicAdd(dst + j, sA0[j]);
                }
            }
        }
        asm volatile("" ::: "memory");
        if (*reinterpret_cast<volatile int*>(sFlag))
            attn4_exact_tail<LP, NHD>(smem, p.bits, nullptr, KMODE == 3 ? p.align_map : nullptr, p.ctx, p.align_t, S, H, p.A, n, a0, tid);
    }
    trace(6);
    __syncthreads();        // the images and tables are dead: the next tile's tables / prologue may overwrite them
    trace(7);
    ++trace_it;
    }   // tiles
}

template <int MODE, int LP, int DROP, int NH = 2, int DUMPV = 0, int FOLD = 0>
int launch_attn4d(const AttnArgs& p, hipStream_t st) {
    typedef A4T<LP, NH> A4;
#ifndef MODCR_TUNING
    static_assert(FOLD == 0, "the LayerNorm-fold prototype exists in the tuning library only");
#endif
    constexpr int SMEM_ = FOLD ? A4::SMEM_FOLD : A4::SMEM;
    if constexpr (NH == 2 && MODE != 0 && LP != 256 && DUMPV == 0) {
        if (p.dump && !modcr_knob_set("MODCR_ATTN_DUMP_BLOCK")) return launch_attn4d<MODE, LP, DROP, NH, 1>(p, st);      // (knob: tuning build, A/B)
    }
    static bool configured_dev[MODCR_MAX_DEV] = {};
    bool& configured = configured_dev[modcr_device_index()];
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qkv_attn4_kernel<MODE, LP, DROP, NH, DUMPV A4_FOLD_ARG>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_);
        if (e != hipSuccess) {
            modcr_set_error("qkv_attn4: cannot reserve %d bytes of LDS: %s", SMEM_, hipGetErrorString(e));
            return MODCR_ERR_LAUNCH;
        }
        configured = true;
    }
    const int ncu = modcr_device_cus() >= 8 ? (modcr_device_cus() & ~7) : 256;
    const int nopersist = modcr_knob_set("MODCR_ATTN_NOPERSIST");          // tuning build only
    const int ntiles = p.N * (p.A / NH);
    const int grid = (ntiles <= ncu || nopersist || MODE == 0) ? ntiles : ncu;
    launch_timed(qkv_attn4_kernel<MODE, LP, DROP, NH, DUMPV A4_FOLD_ARG>, dim3(grid), dim3(A4::NT), (size_t)SMEM_, st, p);
    return modcr_check_launch("qkv_attn4");
}
template <int MODE, int LP, int NH = 2>
int launch_attn4(const AttnArgs& p, hipStream_t st) {
    // the streaming variants carry the dropout masking as a template flag (eval-mode code unchanged); the generic
    // variant (MODE 0) always ends in the exact pass, which takes the threshold at run time
    if (MODE != 0 && p.drop_on) return launch_attn4d<MODE, LP, (MODE != 0), NH>(p, st);
    return launch_attn4d<MODE, LP, 0, NH>(p, st);
}

#ifdef MODCR_TUNING
// LayerNorm-fold PROTOTYPE (tuning library only; tools/proto_ln_fold.py): the key-mask call of the 192-token tile on PRE-LayerNorm rows.
//   pre [N,S,H] bf16, wfold [3H,H] = bf16(gamma o Wqkv), d [3H] = Wqkv beta + bqkv, c [3H] = row sums of wfold (as the MFMA sees them),
//   row_stats [N*S][2] = (rstd, rstd * mu) of every row of pre
extern "C" int modcr_tuning_qkv_attn_fold_fwd(const void* pre, const void* wfold, const float* d, const float* c, const float* row_stats,
                                              const float* key_mask, void* ctx, int32_t N, int32_t S, int32_t H, int32_t A, float attn_p,
                                              uint64_t seed, uint64_t offset, modcr_stream_t stream) {
    MODCR_REQUIRE(pre && wfold && d && c && row_stats && key_mask && ctx, "qkv_attn_fold_fwd: null pointer");
    MODCR_REQUIRE(S > 128 && S <= 192 && (A % 2) == 0 && H == A * 64 && (H % 128) == 0, "qkv_attn_fold_fwd: the 192-token tile only");
    AttnArgs p;
    p.x = (const bf16*)pre; p.hist = nullptr; p.wqkv = (const bf16*)wfold; p.bqkv = d; p.key_mask = key_mask; p.bits = nullptr; p.chunk_id = nullptr;
    p.ctx = (bf16*)ctx; p.probs = nullptr; p.align_map = nullptr; p.lse = nullptr; p.dump = nullptr;
    p.N = N; p.S = S; p.P = 0; p.H = H; p.A = A; p.chunk_t = 0; p.align_t = 0; p.hconc = 3; p.debug = modcr_knob_int("MODCR_ATTN_DEBUG", 0);
    const AttnDrop dr = attn_drop(attn_p, seed, offset);
    p.drop_thr2 = dr.thr2(); p.drop_on = dr.thr16 != 0; p.drop_key = dr.key; p.drop_keep = dr.keep; p.side_post_drop = 0;
    p.row_stats = row_stats; p.cfold = c;
    return attn_p > 0.f ? launch_attn4d<1, 192, 1, 2, 0, 1>(p, (hipStream_t)stream) : launch_attn4d<1, 192, 0, 2, 0, 1>(p, (hipStream_t)stream);
}
#endif

// [prefix ; x] rows of every sequence as one buffer (the tile kernels stage their token rows from ONE base + 32-bit offsets):
// out [N, P + S, H] <- hist [N, P, H], x [N, S, H], 16-byte pieces
__global__ __launch_bounds__(256) void concat_prefix_kernel(const bf16* hist, const bf16* x, bf16* out, int N, int P, int S, int H) {
    const int hv = H >> 3, L = P + S;
    const int64_t total = (int64_t)N * L * hv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % hv);
        const int64_t row = i / hv;
        const int r = (int)(row % L);
        const int64_t n = row / L;
        const bf16* src = r < P ? hist + (n * P + r) * H : x + (n * S + (r - P)) * H;
        reinterpret_cast<uint4*>(out)[i] = reinterpret_cast<const uint4*>(src)[c];
    }
}

// ---- fp32 parity core: one block per (n, head); K_h and V_h in LDS, one query per wave-iteration
struct AttnF32Args {
    const float* qkv_x;   // [N,S,3H]
    const float* qkv_h;   // [N,P,3H] or null
    const float* key_mask; const uint32_t* bits;
    float* ctx; float* probs; float* align_map;
    int N, S, P, H, A, align_t;
    // attention-probability dropout (attn_common.h; the same mask as the bf16 kernels): 0 = off, else round(p * 2^16); side outputs after it?
    uint32_t drop_thr16; uint64_t drop_key; float drop_keep; int side_post_drop;
};

__global__ __launch_bounds__(256) void attn_f32_kernel(AttnF32Args p) {
    extern __shared__ float sm[];
    const int S = p.S, P = p.P, L = P + S, H = p.H;
    float* sK = sm;                  // L x 65
    float* sV = sK + (size_t)L * 65; // L x 65
    float* sQ = sV + (size_t)L * 65; // 4 x 64
    float* sP = sQ + 256;            // 4 x L
    const int n = blockIdx.x / p.A, a = blockIdx.x % p.A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int idx = tid; idx < L * 64; idx += 256) {
        const int j = idx >> 6, d = idx & 63;
        const float* row = (j < P) ? p.qkv_h + ((int64_t)n * P + j) * 3 * H
                                   : p.qkv_x + ((int64_t)n * S + (j - P)) * 3 * H;
        sK[j * 65 + d] = row[H + a * 64 + d];
        sV[j * 65 + d] = row[2 * H + a * 64 + d];
    }
    __syncthreads();
    const int LW = (L + 31) >> 5;
    for (int i = wave; i < S; i += 4) {
        sQ[wave * 64 + lane] = p.qkv_x[((int64_t)n * S + i) * 3 * H + a * 64 + lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float sv[4];
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = lane + 64 * c;
            sv[c] = -INFINITY;
            if (j < L) {
                float s = 0.f;
                for (int d = 0; d < 64; ++d) s = fmaf(sQ[wave * 64 + d], sK[j * 65 + d], s);
                s = s / 8.0f;
                bool see;
                if (p.bits) see = (p.bits[((int64_t)n * S + i) * LW + (j >> 5)] >> (j & 31)) & 1u;
                else see = p.key_mask[(int64_t)n * L + j] != 0.f;
                s += see ? 0.f : MODCR_NEG;
                sv[c] = s;
                mx = fmaxf(mx, s);
            }
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = lane + 64 * c;
            if (j < L) { sv[c] = expf(sv[c] - mx); sum += sv[c]; }
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = lane + 64 * c;
            if (j < L) {
                const float pj = sv[c] / sum;
                float pd = pj;                              // after nn.Dropout (modeling_bert.py:69): what multiplies V
                if (p.drop_thr16) {
                    uint32_t hx, hy;
                    attn_drop_words((uint32_t)((n * p.A + a) * attn_drop_stride(ATTN_DROP_NARROW_KEYS) + i), j >> 2, p.drop_key, hx, hy);
                    pd = attn_keep_field(hx, hy, j & 3, p.drop_thr16) ? pj * p.drop_keep : 0.f;
                }
                sP[wave * L + j] = pd;
                const float side = p.side_post_drop ? pd : pj;
                if (p.probs) p.probs[(((int64_t)n * p.A + a) * S + i) * L + j] = side;
                if (p.align_map && i < p.align_t && j >= P + p.align_t)
                    atomicAdd(p.align_map + ((int64_t)n * p.align_t + i) * (S - p.align_t) + (j - P - p.align_t), side);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        float o = 0.f;
        for (int j = 0; j < L; ++j) o = fmaf(sP[wave * L + j], sV[j * 65 + lane], o);
        p.ctx[((int64_t)n * S + i) * H + a * 64 + lane] = o;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

}  // namespace

extern "C" int modcr_time_next_attn(void* start_event, void* stop_event) {
    g_time_start = (hipEvent_t)start_event;
    g_time_stop = (hipEvent_t)stop_event;
    return MODCR_OK;
}

// bytes of modcr_qkv_attn_lse_fwd's qkv_dump: [N][A][3][LP][64] bf16 with LP = the forward's token tile (0 = no dump at this S)
extern "C" int64_t modcr_qkv_attn_dump_bytes(int32_t N, int32_t S, int32_t A) {
    if (S <= 64 || S > 192) return 0;
    return (int64_t)N * A * 3 * (S <= 128 ? 128 : 192) * 64 * 2;
}

extern "C" int64_t modcr_qkv_attn_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    if (dtype == MODCR_BF16 && P + S > 256) return (int64_t)N * (P + S) * 3 * H * 2;  // q | k | v rows for attn_long.hip
    if (dtype == MODCR_BF16) return P > 0 ? (int64_t)N * (P + S) * H * 2 : 0;      // [prefix ; x] rows for the tile kernels
    return (int64_t)N * (S + P) * 3 * H * (int64_t)sizeof(float);
}

extern "C" int64_t modcr_qkv_attn_bias_workspace(int32_t N, int32_t S, int32_t P, int32_t H, int32_t dtype) {
    return (int64_t)N * (P + S) * 3 * H * (dtype == MODCR_BF16 ? 2 : 4);     // q | k | v rows of [x ; hist] at every key count
}

namespace {

// What validation and routing look at: the scalars of a forward call and which optional arguments it gives (MODCR_ATTN_HAS_*).
// who = the entry's name in the messages; ws_bytes = 0 without a workspace.
struct AttnCall {
    const char* who;
    int32_t present, chunk_t, align_t, N, S, P, H, A; float attn_p; int32_t flags; int64_t ws_bytes; bool ws_aligned16; int32_t dtype;
    bool wide_dropout = false;      // attention dropout above 256 keys is served (modcr_qkv_attn_long_drop_fwd: the wide counter layout)
};

int attn_present(const void* dense_mask_bits, const void* chunk_id, const void* probs, const void* align_map, const void* lse, const void* qkv_dump) {
    return (dense_mask_bits ? MODCR_ATTN_HAS_DENSE_MASK : 0) | (chunk_id ? MODCR_ATTN_HAS_CHUNK_ID : 0) | (probs ? MODCR_ATTN_HAS_PROBS : 0) |
           (align_map ? MODCR_ATTN_HAS_ALIGN_MAP : 0) | (lse ? MODCR_ATTN_HAS_LSE : 0) | (qkv_dump ? MODCR_ATTN_HAS_QKV_DUMP : 0);
}

// The argument checks every forward entry shares.  given = x, wqkv, bqkv and ctx are there; aligned16 = x, wqkv, ctx and hist (P > 0)
// lie on 16 bytes (looked at in bf16 only).
int attn_fwd_setup(const AttnCall& c, bool given, bool has_hist, bool aligned16) {
    const char* who = c.who;
    const bool bias = c.present & MODCR_ATTN_HAS_BIAS, chunk = c.present & MODCR_ATTN_HAS_CHUNK_ID, align = c.present & MODCR_ATTN_HAS_ALIGN_MAP;
    MODCR_REQUIRE(given, "%s: null pointer", who);
    MODCR_REQUIRE((c.flags & ~MODCR_ATTN_SIDE_POST_DROPOUT) == 0, "%s: unknown flags 0x%x", who, c.flags);
    MODCR_REQUIRE(c.dtype == MODCR_BF16 || c.dtype == MODCR_F32, "%s: unknown dtype %d", who, c.dtype);
    MODCR_REQUIRE(c.N > 0 && c.S > 0 && c.P >= 0 && c.A > 0, "%s: bad shape", who);
    MODCR_REQUIRE(c.H == c.A * 64, "%s: head size must be 64 (H=%d, A=%d)", who, c.H, c.A);
    const int L = c.P + c.S;
    if (L > 512 || (c.attn_p > 0.f && L > 256 && !c.wide_dropout)) {
        if (L > 512) modcr_set_error("%s: P+S=%d exceeds the 512-key limit of the attention forward", who, L);
        else modcr_set_error("%s: attention-probability dropout (p=%g) is not implemented above 256 keys (P+S=%d)", who, c.attn_p, L);
        return MODCR_ERR_UNSUPPORTED;
    }
    // (the wide counter layout: (n A + head) x 512 rows x 4 counters in 32 bits)
    MODCR_REQUIRE(!(c.attn_p > 0.f && L > 256) || (int64_t)c.N * c.A <= ATTN_DROP_WIDE_MAX_NA,
                  "%s: N * A = %lld (N=%d, A=%d) exceeds the 2^21 (sequence, head) pairs of the wide dropout counter", who, (long long)c.N * c.A, c.N, c.A);
    // (above 256 keys the binary-mask entries have only ever asked whether p > 0: anything else is "no dropout" there)
    MODCR_REQUIRE((L > 256 && !bias) || (c.attn_p >= 0.f && c.attn_p < 1.f), "%s: attention dropout p=%g out of [0, 1)", who, c.attn_p);
    MODCR_REQUIRE(c.P == 0 || has_hist, "%s: P=%d but hist is null", who, c.P);
    MODCR_REQUIRE(!chunk || (c.chunk_t > 0 && c.chunk_t <= c.S), "%s: chunk_t=%d out of range", who, c.chunk_t);
    MODCR_REQUIRE(!align || (c.align_t > 0 && c.align_t < c.S), "%s: align_t=%d out of range", who, c.align_t);
    MODCR_REQUIRE(!(bias || L > 256) || (c.N <= 65535 && c.A <= 65535), "%s: grid of N=%d sequences x A=%d heads too large", who, c.N, c.A);   // (the streaming core's)
    MODCR_REQUIRE(c.dtype != MODCR_BF16 || aligned16, "%s(bf16): 16-byte alignment", who);
    return MODCR_OK;
}

// modcr_qkv_attn_opt_fwd's own checks, after the shared ones
int attn_opt_checks(const AttnCall& c, bool has_mask, bool dump_aligned16) {
    MODCR_REQUIRE(has_mask, "%s: need key_mask or dense_mask_bits", c.who);
    MODCR_REQUIRE(!(c.present & MODCR_ATTN_HAS_QKV_DUMP) || c.P + c.S > 256 ||
                      ((c.present & MODCR_ATTN_HAS_LSE) && c.P == 0 && c.S > 64 && c.S <= 192 && dump_aligned16),
                  "%s: the q|k|v dump comes with lse, without prefix rows, for 64 < S <= 192 (S=%d P=%d)", c.who, c.S, c.P);
    return MODCR_OK;
}

// modcr_qkv_attn_bias_fwd's own checks (b: its bias / head_mask arguments)
int attn_bias_checks(const char* who, const AttnLongArgs& b, bool bits = false) {
    MODCR_REQUIRE(b.bias || b.head_mask || bits, "%s: neither bias nor head_mask (that call belongs to modcr_qkv_attn_opt_fwd)", who);
    MODCR_REQUIRE(b.bias_sn >= 0 && b.bias_sa >= 0 && b.bias_sq >= 0 && b.head_mask_sn >= 0, "%s: negative stride", who);
    MODCR_REQUIRE(((uintptr_t)b.bias & 3) == 0 && ((uintptr_t)b.head_mask & 3) == 0, "%s: bias / head_mask not 4-byte aligned", who);
    return MODCR_OK;
}

// The route of a validated forward call (every forward entry and modcr_qkv_attn_route).  The one place the choice is made:
// family = MODCR_ATTN_ROUTE_*, v = what picks the instantiation (modcr_hip.h: info[1..5]), concat = concat_prefix_kernel runs first,
// rc = MODCR_OK or why no route serves the call (the message is set).  DROP / DUMPV / SIDE of the launchers follow from the pointers
// and stay with them.  The MODCR_ATTN_* knobs read here exist in the tuning build only (common.h).
struct AttnRoute { int rc, family, v[5], concat; };
AttnRoute attn_fwd_route(const AttnCall& c) {
    AttnRoute r = {MODCR_OK, 0, {0, 0, 0, 0, 0}, 0};
    const int N = c.N, S = c.S, P = c.P, H = c.H, A = c.A, L = P + S;
    const bool bf = c.dtype == MODCR_BF16, bias = c.present & MODCR_ATTN_HAS_BIAS, dense = c.present & MODCR_ATTN_HAS_DENSE_MASK,
               chunk = c.present & MODCR_ATTN_HAS_CHUNK_ID, probs = c.present & MODCR_ATTN_HAS_PROBS,
               align = c.present & MODCR_ATTN_HAS_ALIGN_MAP, lse = c.present & MODCR_ATTN_HAS_LSE, rows = c.present & MODCR_ATTN_HAS_ROW_START;
    const bool side_post_drop = c.attn_p > 0.f && (c.flags & MODCR_ATTN_SIDE_POST_DROPOUT);
    auto refuse = [&r](int rc, const char* fmt, auto... a) { modcr_set_error(fmt, a...); r.rc = rc; return r; };
    auto tile = [&r](int nw, int hpw, int occ, int bka, int nslot) { r = {MODCR_OK, MODCR_ATTN_ROUTE_TILE, {nw, hpw, occ, bka, nslot}, 0}; };
    // (prefix rows reach qkv_attn4_kernel through the concatenated copy only)
    auto tile4 = [&r, P](int mode, int lp, int nh) { r = {MODCR_OK, MODCR_ATTN_ROUTE_TILE4, {mode, lp, nh, 0, 0}, P > 0}; };
    // the live-row layout (modcr_qkv_attn_rows_fwd) exists in the streaming variants of qkv_attn4_kernel on the 128- and 192-token
    // tiles only; everything else is refused here and the caller keeps the dense layout
    if (rows && (bias || !bf || P > 0 || L > 192 || probs || (c.present & (MODCR_ATTN_HAS_LSE | MODCR_ATTN_HAS_QKV_DUMP))))
        return refuse(MODCR_ERR_UNSUPPORTED, "%s: the live-row layout takes bf16 calls of at most 192 keys without prefix rows, probabilities, "
                      "lse or q|k|v dump (S=%d P=%d)", c.who, S, P);
    // the streaming core of attn_long.hip over projected rows: above 256 keys (eval mode: no dropout, no row statistics, no q|k|v
    // dump -- those exist for the backward, which stops at 256 keys), and every call of modcr_qkv_attn_bias_fwd
    if (bias || L > 256) {
        if (c.present & (MODCR_ATTN_HAS_LSE | MODCR_ATTN_HAS_QKV_DUMP))
            return refuse(MODCR_ERR_UNSUPPORTED, "%s: row statistics (lse) / q|k|v dump are not produced above 256 keys (P+S=%d): no backward there", c.who, L);
        const int64_t need = bias ? modcr_qkv_attn_bias_workspace(N, S, P, H, c.dtype) : modcr_qkv_attn_workspace(N, S, P, H, c.dtype);
        if (c.ws_bytes < need || !c.ws_aligned16)
            return refuse(MODCR_ERR_INVALID, "%s: workspace %lld < %lld bytes (or unaligned)", c.who, (long long)c.ws_bytes, (long long)need);
        r.family = bf ? MODCR_ATTN_ROUTE_LONG_BF16 : MODCR_ATTN_ROUTE_LONG_F32;
        // (reported only: modcr_launch_attn_long, attn_long.hip, derives the same mode from the arguments attn_fwd fills -- bias or
        // head_mask set, drop_thr16 = attn_thr16(p) >= 1 exactly when p > 0; tools/attn_route_trace.py holds the two together)
        r.v[0] = !bias ? 0 : c.attn_p > 0.f ? 2 : 1;
        return r;
    }
    // the reference returns the probabilities AFTER the dropout (modeling_bert.py:74): a probabilities output comes with
    // MODCR_ATTN_SIDE_POST_DROPOUT (the generic tile variant applies the mask to it); the un-dropped ones are not offered
    if (c.attn_p > 0.f && probs && !side_post_drop)
        return refuse(bf ? MODCR_ERR_UNSUPPORTED : MODCR_ERR_INVALID,
                      "%s%s: a probabilities output under attention-probability dropout needs MODCR_ATTN_SIDE_POST_DROPOUT", c.who, bf ? "" : "(f32)");
    if (!bf) {              // exact-parity core over projected rows
        if (lse) return refuse(MODCR_ERR_INVALID, "%s(f32): row statistics (lse) are written on the bf16 path only", c.who);
        const int64_t need = modcr_qkv_attn_workspace(N, S, P, H, c.dtype);
        if (c.ws_bytes < need) return refuse(MODCR_ERR_INVALID, "%s(f32): workspace %lld < %lld bytes", c.who, (long long)c.ws_bytes, (long long)need);
        r.family = MODCR_ATTN_ROUTE_F32;
        return r;
    }
    const int hpw1 = modcr_knob_int("MODCR_ATTN_HPW1", 0);              // (set: one head per workgroup; 2, 3: A/B variants at 192 rows)
    const bool pair = (A % 2 == 0) && !modcr_knob_set("MODCR_ATTN_HPW1");
    const bool tile4_shape = (H % 128) == 0 && H >= 256 && (int64_t)3 * H * H * 2 < (1ll << 31);     // what qkv_attn4_kernel takes
    // prefix rows (history_state) on the tile kernels: K and V over [prefix ; x] (modeling_bert.py:36-44), queries from x only.
    // The caller's workspace receives the concatenated rows (one copy pass); key-mask / dense-mask calls without side outputs
    // take this route, everything else the older kernel.
    const bool prefix_tiles = P > 0 && L > 64 && (pair || L > 192) && !probs && !align && !chunk && tile4_shape &&
                              c.ws_bytes >= modcr_qkv_attn_workspace(N, S, P, H, c.dtype) && c.ws_aligned16 &&
                              !modcr_knob_set("MODCR_ATTN_NO_PREFIX_TILES") && !modcr_knob_set("MODCR_ATTN_NO_V4") &&
                              !modcr_knob_set("MODCR_ATTN_NO_V4S");
    const bool rows4 = tile4_shape && (P == 0 || prefix_tiles);
    // MODE of qkv_attn4_kernel: 3 = the phase-3 call (dense mask + chunk-mean queries + align map), 0 = the generic variant (a
    // probabilities output, chunk-mean queries / an align map in any other combination), 2 / 1 = dense mask / key mask alone
    const int mode4 = (!probs && align && chunk && dense) ? 3 : (probs || align || chunk) ? 0 : dense ? 2 : 1;
    if (L <= 64) {
        tile(2, pair ? 2 : 1, 2, 64, 2);
    } else if (L <= 128) {  // the 128-token tile (A half = 64 rows = one LDS-DMA piece per wave)
        const int ring32 = modcr_knob_int("MODCR_ATTN_RING32", 0);
        if (pair && rows4 && !modcr_knob_set("MODCR_ATTN_NO_V4S")) tile4(mode4, 128, 2);
        else if (pair && (ring32 == 1 || ring32 == 2)) tile(4, 2, 2, 32, ring32 == 1 ? 4 : 3);
        else tile(4, pair ? 2 : 1, 2, 64, 2);
    } else if (L <= 192) {
        if (pair && rows4 && !modcr_knob_set("MODCR_ATTN_NO_V4")) tile4(mode4, 192, 2);
        else if (!pair && hpw1 == 2) tile(6, 1, 3, 32, 3);        // 2 workgroups per CU
        else if (!pair && hpw1 == 3) tile(6, 1, 3, 32, 2);
        else if (!pair) tile(6, 1, 2, 64, 2);
        else if (modcr_knob_set("MODCR_ATTN_RING64")) tile(6, 2, 3, 64, 2);          // 64-wide K-tiles, 2 slots
        else tile(6, 2, 3, 32, 4);
    } else {
        // 192 < L <= 256 (the VCR / Oscar-large shape class S = 230): the 256-token tile, one head per workgroup; key-mask and
        // dense-mask calls without side outputs, and the phase-3 call when its [T][R] fp32 tile fits the one V^T image (VCR:
        // 194 x 36); a probabilities output, or chunk-mean queries / an align map in any other combination (incl. a larger [T][R]
        // tile): the generic variant of the same tile (exact pass; its align tile lies over K | V^T); prefix rows with any of
        // those: the older kernel
        const bool v4l = !modcr_knob_set("MODCR_ATTN_NO_V4L");
        if (v4l && rows4 && (mode4 == 1 || mode4 == 2)) tile4(mode4, 256, 1);
        else if (v4l && rows4 && P == 0 && mode4 == 3 && (int64_t)c.align_t * (S - c.align_t) * 4 <= (int64_t)64 * A4T<256, 1>::VT_STRIDE) tile4(3, 256, 1);
        else if (v4l && rows4 && P == 0) tile4(0, 256, 1);
        else tile(8, 1, 2, 64, 2);
    }
    if (rows && !(r.family == MODCR_ATTN_ROUTE_TILE4 && r.v[0] >= 1 && r.v[1] <= 192))
        return refuse(MODCR_ERR_UNSUPPORTED, "%s: the live-row layout is served by the key-mask, dense-mask and phase-3 variants of the 128- / 192-token "
                      "tile kernel only (S=%d A=%d H=%d)", c.who, S, A, H);
    // row statistics and post-dropout side outputs come from qkv_attn4_kernel only
    if (r.family == MODCR_ATTN_ROUTE_TILE && lse)
        return refuse(MODCR_ERR_UNSUPPORTED, "%s: no row statistics (lse) on this route (S=%d P=%d A=%d H=%d)", c.who, S, P, A, H);
    if (r.family == MODCR_ATTN_ROUTE_TILE && side_post_drop && (probs || align))
        return refuse(MODCR_ERR_UNSUPPORTED, "%s: post-dropout side outputs on the tile kernels only (S=%d P=%d A=%d H=%d)", c.who, S, P, A, H);
    return r;
}

constexpr int tile_id(int nw, int hpw, int occ, int bka, int nslot) { return (((nw * 4 + hpw) * 4 + occ) * 128 + bka) * 8 + nslot; }
int launch_route_tile(const AttnRoute& r, const AttnArgs& p, hipStream_t st) {
    switch (tile_id(r.v[0], r.v[1], r.v[2], r.v[3], r.v[4])) {
        case tile_id(2, 2, 2, 64, 2): return launch_attn<2, 2, 2, 64, 2>(p, st);
        case tile_id(2, 1, 2, 64, 2): return launch_attn<2, 1, 2, 64, 2>(p, st);
        case tile_id(4, 2, 2, 64, 2): return launch_attn<4, 2, 2, 64, 2>(p, st);
        case tile_id(4, 1, 2, 64, 2): return launch_attn<4, 1, 2, 64, 2>(p, st);
        case tile_id(6, 1, 2, 64, 2): return launch_attn<6, 1, 2, 64, 2>(p, st);
        case tile_id(6, 2, 3, 32, 4): return launch_attn<6, 2, 3, 32, 4>(p, st);
        case tile_id(8, 1, 2, 64, 2): return launch_attn<8, 1, 2, 64, 2>(p, st);
#ifdef MODCR_TUNING             // (A/B variants of the older kernel: instantiated in the tuning library only)
        case tile_id(4, 2, 2, 32, 4): return launch_attn<4, 2, 2, 32, 4>(p, st);
        case tile_id(4, 2, 2, 32, 3): return launch_attn<4, 2, 2, 32, 3>(p, st);
        case tile_id(6, 1, 3, 32, 3): return launch_attn<6, 1, 3, 32, 3>(p, st);
        case tile_id(6, 1, 3, 32, 2): return launch_attn<6, 1, 3, 32, 2>(p, st);
        case tile_id(6, 2, 3, 64, 2): return launch_attn<6, 2, 3, 64, 2>(p, st);
#endif
    }
    modcr_set_error("qkv_attn_fwd: no instantiation NW=%d HPW=%d OCC=%d BKA=%d NSLOT=%d", r.v[0], r.v[1], r.v[2], r.v[3], r.v[4]);
    return MODCR_ERR_UNSUPPORTED;
}
template <int LP, int NH> int launch_route_tile4(int mode, const AttnArgs& p, hipStream_t st) {
    switch (mode) {
        case 0: return launch_attn4<0, LP, NH>(p, st);
        case 1: return launch_attn4<1, LP, NH>(p, st);
        case 2: return launch_attn4<2, LP, NH>(p, st);
    }
    return launch_attn4<3, LP, NH>(p, st);
}

// x rows [N*S][3H], then the prefix rows [N*P][3H], projected into the workspace; chunk-mean over the query columns
int attn_project(const void* x, const void* hist, const void* wqkv, const float* bqkv, const int32_t* chunk_id, int32_t chunk_t, int N, int S,
                 int P, int H, void* workspace, int32_t dtype, modcr_stream_t stream, const void*& qx, const void*& qh) {
    char* rx = (char*)workspace;
    char* rh = rx + (int64_t)N * S * 3 * H * (dtype == MODCR_BF16 ? 2 : 4);
    int rc = modcr_linear_fwd(x, H, wqkv, H, bqkv, nullptr, 0, 0, rx, 3 * H, N * S, 3 * H, H, MODCR_ACT_NONE, dtype, dtype, stream);
    if (rc != MODCR_OK) return rc;
    if (P > 0) {
        rc = modcr_linear_fwd(hist, H, wqkv, H, bqkv, nullptr, 0, 0, rh, 3 * H, N * P, 3 * H, H, MODCR_ACT_NONE, dtype, dtype, stream);
        if (rc != MODCR_OK) return rc;
    }
    if (chunk_id) {
        rc = modcr_chunk_mean_q_fwd(rx, 3 * H, (int64_t)S * 3 * H, chunk_id, N, chunk_t, H, dtype, stream);
        if (rc != MODCR_OK) return rc;
    }
    qx = rx; qh = P > 0 ? rh : nullptr;
    return MODCR_OK;
}

int launch_attn_f32(const AttnF32Args& f, hipStream_t st) {
    const int L = f.P + f.S;
    const size_t smem = ((size_t)2 * L * 65 + 256 + 4 * (size_t)L) * sizeof(float);
    static bool configured_dev[MODCR_MAX_DEV] = {};
    bool& configured = configured_dev[modcr_device_index()];
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) {
            modcr_set_error("qkv_attn(f32): cannot reserve LDS: %s", hipGetErrorString(e));
            return MODCR_ERR_LAUNCH;
        }
        configured = true;
    }
    hipLaunchKernelGGL(attn_f32_kernel, dim3(f.N * f.A), dim3(256), smem, st, f);
    return modcr_check_launch("attn_f32");
}

// Every forward entry: setup, route, the route's arguments, launch.  bias = the bias / head_mask arguments of modcr_qkv_attn_bias_fwd.
// lse (or NULL): [N, A, S] fp32, log2 of every query row's sum of exp2(log2e x score) -- the row statistics the five-product
// backward rebuilds the probabilities from.  flags: modcr_hip.h (MODCR_ATTN_SIDE_POST_DROPOUT: modeling_bert.py:69-74, v10:94-106).
int attn_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* key_mask, const uint32_t* dense_mask_bits,
             const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs, float* align_map, int32_t align_t, float* lse, void* qkv_dump,
             int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p, uint64_t seed, uint64_t offset, int32_t flags,
             void* workspace, int64_t workspace_bytes, int32_t dtype, modcr_stream_t stream, const AttnLongArgs* bias = nullptr,
             const int32_t* row_start = nullptr, bool wide_dropout = false) {
    // (wide_dropout: modcr_qkv_attn_long_drop_fwd; it shows, name included, only where it changes the call: dropout above 256 keys)
    const bool wide = wide_dropout && bias && (int64_t)P + S > 256 && attn_p > 0.f;
    AttnCall c = {wide ? "qkv_attn_long_drop_fwd" : bias ? "qkv_attn_bias_fwd" : row_start ? "qkv_attn_rows_fwd" : "qkv_attn_fwd",
                        (bias ? MODCR_ATTN_HAS_BIAS : 0) | (row_start ? MODCR_ATTN_HAS_ROW_START : 0) | attn_present(dense_mask_bits, chunk_id, probs, align_map, lse, qkv_dump), chunk_t, align_t,
                        N, S, P, H, A, attn_p, flags, workspace ? workspace_bytes : 0, modcr_aligned16(workspace), dtype};
    c.wide_dropout = wide;
    int rc = attn_fwd_setup(c, x && wqkv && bqkv && ctx, hist != nullptr,
                            modcr_aligned16(x) && modcr_aligned16(wqkv) && modcr_aligned16(ctx) && (P == 0 || modcr_aligned16(hist)));
    if (rc == MODCR_OK) rc = bias ? attn_bias_checks(c.who, *bias, dense_mask_bits != nullptr) : attn_opt_checks(c, key_mask || dense_mask_bits, modcr_aligned16(qkv_dump));
    if (rc != MODCR_OK) return rc;
    const AttnRoute r = attn_fwd_route(c);
    if (r.rc != MODCR_OK) return r.rc;
    hipStream_t st = (hipStream_t)stream;
    const AttnDrop d = attn_drop(attn_p, seed, offset);     // the same mask on every route, so that they can be compared
    const int side_post_drop = (attn_p > 0.f && (flags & MODCR_ATTN_SIDE_POST_DROPOUT)) ? 1 : 0;
    if (r.family == MODCR_ATTN_ROUTE_TILE || r.family == MODCR_ATTN_ROUTE_TILE4) {
        AttnArgs p;
        p.x = (const bf16*)x; p.hist = (const bf16*)hist; p.wqkv = (const bf16*)wqkv; p.bqkv = bqkv;
        p.key_mask = key_mask; p.bits = dense_mask_bits; p.chunk_id = chunk_id;
        p.ctx = (bf16*)ctx; p.probs = probs; p.align_map = align_map; p.lse = lse; p.dump = (bf16*)qkv_dump;
        p.N = N; p.S = S; p.P = P; p.H = H; p.A = A; p.chunk_t = chunk_t; p.align_t = align_t;
        p.drop_on = d.thr16 != 0; p.drop_thr2 = d.thr2(); p.drop_key = d.key; p.drop_keep = d.keep;
        p.side_post_drop = side_post_drop;
        p.row_start = row_start;
        // knobs below: tuning build only (common.h); the product library takes the defaults
        p.debug = modcr_knob_int("MODCR_ATTN_DEBUG", 0);
#ifdef MODCR_TUNING
        if (getenv("MODCR_ATTN_TRACE_PTR")) p.trace = reinterpret_cast<unsigned long long*>(strtoull(getenv("MODCR_ATTN_TRACE_PTR"), nullptr, 0));
#endif
        p.hconc = modcr_knob_int("MODCR_ATTN_HCONC", 3);     // tile kernels: 3 head pairs at a time per XCD (measured 166 vs 168 us; FETCH_SIZE: profiles/)
        if (r.concat) {
            const int64_t pieces = (int64_t)N * (P + S) * (H >> 3);
            const int grid = (int)((pieces + 255) / 256 < 16384 ? (pieces + 255) / 256 : 16384);
            hipLaunchKernelGGL(concat_prefix_kernel, dim3(grid), dim3(256), 0, st, p.hist, p.x, (bf16*)workspace, N, P, S, H);
            rc = modcr_check_launch("concat_prefix");
            if (rc != MODCR_OK) return rc;
            p.x = (const bf16*)workspace;
        }
        if (r.family == MODCR_ATTN_ROUTE_TILE) return launch_route_tile(r, p, st);
        if (r.v[1] == 128) return launch_route_tile4<128, 2>(r.v[0], p, st);
        return r.v[1] == 192 ? launch_route_tile4<192, 2>(r.v[0], p, st) : launch_route_tile4<256, 1>(r.v[0], p, st);
    }
    const void *qx, *qh;
    rc = attn_project(x, hist, wqkv, bqkv, chunk_id, chunk_t, N, S, P, H, workspace, dtype, stream, qx, qh);
    if (rc != MODCR_OK) return rc;
    if (r.family == MODCR_ATTN_ROUTE_F32) {
        AttnF32Args f;
        f.qkv_x = (const float*)qx; f.qkv_h = (const float*)qh; f.key_mask = key_mask; f.bits = dense_mask_bits;
        f.ctx = (float*)ctx; f.probs = probs; f.align_map = align_map;
        f.N = N; f.S = S; f.P = P; f.H = H; f.A = A; f.align_t = align_t;
        f.drop_thr16 = d.thr16; f.drop_key = d.key; f.drop_keep = d.keep; f.side_post_drop = side_post_drop;
        return launch_attn_f32(f, st);
    }
    AttnLongArgs g = bias ? *bias : AttnLongArgs{};
    g.qx = qx; g.qh = qh; g.key_mask = key_mask; g.bits = dense_mask_bits;
    g.ctx = ctx; g.probs = probs; g.align_map = align_map;
    g.N = N; g.S = S; g.P = P; g.H = H; g.A = A; g.align_t = align_t;
    g.drop_thr16 = d.thr16; g.drop_key = d.key; g.drop_keep = d.keep; g.side_post_drop = side_post_drop;
    g.bits_on_bias = bias && dense_mask_bits;               // (modcr_qkv_attn_long_align_fwd only: the other bias entries pass no bits)
    hipEvent_t ev0 = g_time_start, ev1 = g_time_stop;       // the measurement hook times the core, not the projection
    g_time_start = g_time_stop = nullptr;
    return modcr_launch_attn_long(g, dtype, st, ev0, ev1);
}

}  // namespace

extern "C" int modcr_qkv_attn_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* key_mask,
                                  const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs,
                                  float* align_map, int32_t align_t, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, void* workspace,
                                  int64_t workspace_bytes, int32_t dtype, modcr_stream_t stream) {
    return attn_fwd(x, hist, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, ctx, probs, align_map, align_t, nullptr, nullptr,
                    N, S, P, H, A, 0.f, 0, 0, 0, workspace, workspace_bytes, dtype, stream);
}

extern "C" int modcr_qkv_attn_dropout_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* key_mask,
                                          const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs,
                                          float* align_map, int32_t align_t, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                          uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                          modcr_stream_t stream) {
    return attn_fwd(x, hist, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, ctx, probs, align_map, align_t, nullptr, nullptr,
                    N, S, P, H, A, attn_p, seed, offset, 0, workspace, workspace_bytes, dtype, stream);
}

extern "C" int modcr_qkv_attn_lse_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* key_mask,
                                      const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs,
                                      float* align_map, int32_t align_t, float* lse, void* qkv_dump, int32_t N, int32_t S, int32_t P, int32_t H,
                                      int32_t A, float attn_p, uint64_t seed, uint64_t offset, void* workspace, int64_t workspace_bytes,
                                      int32_t dtype, modcr_stream_t stream) {
    return attn_fwd(x, hist, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, ctx, probs, align_map, align_t, lse, qkv_dump,
                    N, S, P, H, A, attn_p, seed, offset, 0, workspace, workspace_bytes, dtype, stream);
}

extern "C" int modcr_qkv_attn_opt_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* key_mask,
                                      const uint32_t* dense_mask_bits, const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs,
                                      float* align_map, int32_t align_t, float* lse, void* qkv_dump, int32_t N, int32_t S, int32_t P, int32_t H,
                                      int32_t A, float attn_p, uint64_t seed, uint64_t offset, int32_t flags, void* workspace,
                                      int64_t workspace_bytes, int32_t dtype, modcr_stream_t stream) {
    return attn_fwd(x, hist, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, ctx, probs, align_map, align_t, lse, qkv_dump,
                    N, S, P, H, A, attn_p, seed, offset, flags, workspace, workspace_bytes, dtype, stream);
}

// The key-mask / dense-mask / phase-3 forward over the live-row layout (AttnArgs::row_start): x and ctx hold sequence n's first
// L_n = row_start[n + 1] - row_start[n] rows from row row_start[n] on, inside buffers of N * S rows.  Same kernels, same arithmetic.
extern "C" int modcr_qkv_attn_rows_fwd(const void* x, const void* wqkv, const float* bqkv, const float* key_mask, const uint32_t* dense_mask_bits,
                                       const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* align_map, int32_t align_t,
                                       const int32_t* row_start, int32_t N, int32_t S, int32_t H, int32_t A, float attn_p, uint64_t seed,
                                       uint64_t offset, int32_t flags, int32_t dtype, modcr_stream_t stream) {
    MODCR_REQUIRE(row_start && ((uintptr_t)row_start & 3) == 0, "qkv_attn_rows_fwd: row_start is null or not 4-byte aligned");
    MODCR_REQUIRE((int64_t)N * S < (1ll << 31), "qkv_attn_rows_fwd: N * S = %lld rows exceed the int32 row table", (long long)N * S);
    return attn_fwd(x, nullptr, wqkv, bqkv, key_mask, dense_mask_bits, chunk_id, chunk_t, ctx, nullptr, align_map, align_t, nullptr, nullptr,
                    N, S, 0, H, A, attn_p, seed, offset, flags, nullptr, 0, dtype, stream, nullptr, row_start);
}

// Attention forward with an additive fp32 bias (any float mask, broadcastable over sequence / head / query) and / or a per-head
// multiplier, P + S <= 512: the bias variant of the streaming core (mode 1, or 2 with dropout) at every key count.
extern "C" int modcr_qkv_attn_bias_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* bias, int64_t bias_stride_n,
                                       int64_t bias_stride_a, int64_t bias_stride_q, const float* head_mask, int64_t head_mask_stride_n,
                                       const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs, float* align_map, int32_t align_t,
                                       int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p, uint64_t seed, uint64_t offset,
                                       int32_t flags, void* workspace, int64_t workspace_bytes, int32_t dtype, modcr_stream_t stream) {
    AttnLongArgs b = {};
    b.bias = bias; b.bias_sn = bias_stride_n; b.bias_sa = bias_stride_a; b.bias_sq = bias_stride_q;
    b.head_mask = head_mask; b.head_mask_sn = head_mask_stride_n;
    return attn_fwd(x, hist, wqkv, bqkv, nullptr, nullptr, chunk_id, chunk_t, ctx, probs, align_map, align_t, nullptr, nullptr,
                    N, S, P, H, A, attn_p, seed, offset, flags, workspace, workspace_bytes, dtype, stream, &b);
}

// modcr_qkv_attn_bias_fwd with attention-probability dropout above 256 keys (opt-in): the same arguments, the same workspace
// (modcr_qkv_attn_bias_workspace).  At P + S <= 256 or attn_p = 0 it is that entry's call; above, MODE 2 of the streaming core runs
// under the wide counter layout of attn_common.h (row stride 512), N * A <= 2^21.
extern "C" int modcr_qkv_attn_long_drop_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* bias,
                                            int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q, const float* head_mask,
                                            int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs,
                                            float* align_map, int32_t align_t, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                            uint64_t seed, uint64_t offset, int32_t flags, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                            modcr_stream_t stream) {
    AttnLongArgs b = {};
    b.bias = bias; b.bias_sn = bias_stride_n; b.bias_sa = bias_stride_a; b.bias_sq = bias_stride_q;
    b.head_mask = head_mask; b.head_mask_sn = head_mask_stride_n;
    return attn_fwd(x, hist, wqkv, bqkv, nullptr, nullptr, chunk_id, chunk_t, ctx, probs, align_map, align_t, nullptr, nullptr,
                    N, S, P, H, A, attn_p, seed, offset, flags, workspace, workspace_bytes, dtype, stream, &b, nullptr, true);
}

// modcr_qkv_attn_long_drop_fwd with the dense mask bits of modcr_build_phase_mask / modcr_pack_mask_bits on top of the bias (opt-in:
// training seq_enc above 256 keys): the BITS instantiations of the streaming core, 0 / -10000 per (query, key) joined to the bias.
// Without mask_bits it is modcr_qkv_attn_long_drop_fwd's call.
extern "C" int modcr_qkv_attn_long_align_fwd(const void* x, const void* hist, const void* wqkv, const float* bqkv, const float* bias,
                                             int64_t bias_stride_n, int64_t bias_stride_a, int64_t bias_stride_q, const float* head_mask,
                                             int64_t head_mask_stride_n, const int32_t* chunk_id, int32_t chunk_t, void* ctx, float* probs,
                                             float* align_map, int32_t align_t, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A, float attn_p,
                                             uint64_t seed, uint64_t offset, int32_t flags, void* workspace, int64_t workspace_bytes, int32_t dtype,
                                             modcr_stream_t stream, const uint32_t* mask_bits) {
    if (!mask_bits)
        return modcr_qkv_attn_long_drop_fwd(x, hist, wqkv, bqkv, bias, bias_stride_n, bias_stride_a, bias_stride_q, head_mask, head_mask_stride_n,
                                            chunk_id, chunk_t, ctx, probs, align_map, align_t, N, S, P, H, A, attn_p, seed, offset, flags, workspace,
                                            workspace_bytes, dtype, stream);
    MODCR_REQUIRE(P == 0 && !hist, "qkv_attn_long_align_fwd: no mask_bits with prefix rows (P=%d, hist %s)", P, hist ? "given" : "null");
    if (S <= 256) {
        modcr_set_error("qkv_attn_long_align_fwd: mask_bits on the bias route start above 256 keys (S=%d): up to 256 they belong to "
                        "modcr_qkv_attn_opt_fwd", S);
        return MODCR_ERR_UNSUPPORTED;
    }
    MODCR_REQUIRE(((uintptr_t)mask_bits & 3) == 0, "qkv_attn_long_align_fwd: mask_bits not 4-byte aligned");
    AttnLongArgs b = {};
    b.bias = bias; b.bias_sn = bias_stride_n; b.bias_sa = bias_stride_a; b.bias_sq = bias_stride_q;
    b.head_mask = head_mask; b.head_mask_sn = head_mask_stride_n;
    return attn_fwd(x, nullptr, wqkv, bqkv, nullptr, mask_bits, chunk_id, chunk_t, ctx, probs, align_map, align_t, nullptr, nullptr,
                    N, S, 0, H, A, attn_p, seed, offset, flags, workspace, workspace_bytes, dtype, stream, &b, nullptr, true);
}

extern "C" int modcr_qkv_attn_route(int32_t present, int32_t chunk_t, int32_t align_t, int32_t N, int32_t S, int32_t P, int32_t H, int32_t A,
                                    float attn_p, int32_t flags, int64_t workspace_bytes, int32_t workspace_aligned16, int32_t dtype, int32_t* info) {
    MODCR_REQUIRE(info, "qkv_attn_route: null info");
    const bool bias = present & MODCR_ATTN_HAS_BIAS;
    MODCR_REQUIRE(!bias || !(present & (MODCR_ATTN_HAS_DENSE_MASK | MODCR_ATTN_HAS_LSE | MODCR_ATTN_HAS_QKV_DUMP)),
                  "qkv_attn_route: modcr_qkv_attn_bias_fwd takes no dense_mask_bits, lse or qkv_dump");
    const AttnCall c = {bias ? "qkv_attn_bias_fwd" : (present & MODCR_ATTN_HAS_ROW_START) ? "qkv_attn_rows_fwd" : "qkv_attn_fwd", present, chunk_t, align_t, N, S, P, H, A, attn_p, flags, workspace_bytes,
                        workspace_aligned16 != 0, dtype};
    int rc = attn_fwd_setup(c, true, true, true);
    if (rc == MODCR_OK && !bias) rc = attn_opt_checks(c, true, true);
    if (rc != MODCR_OK) return rc;
    const AttnRoute r = attn_fwd_route(c);
    if (r.rc != MODCR_OK) return r.rc;
    info[0] = r.family;
    for (int i = 0; i < 5; ++i) info[1 + i] = r.v[i];
    info[6] = r.concat;
    return MODCR_OK;
}
