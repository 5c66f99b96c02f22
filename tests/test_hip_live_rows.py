"""The live-row layout of the frozen encoder passes (include/modcr_hip.h: modcr_qkv_attn_rows_fwd; modcr_hip.LiveRows).

On live rows every kernel does the padded route's arithmetic on the padded route's operands with the padded route's dropout
decisions, so every comparison here is EQUALITY against the padded call on the same inputs -- no tolerance anywhere.

Shapes: H = 256, A = 4 (the smallest the tile kernels accept), N = 6 sequences, (T, R) = (24, 56) -> S = 80 / 57 and (40, 100) ->
S = 140 / 101: the 128- and the 192-token tile.  Region counts per sequence: R, 0, 1, R - 1 and one that makes T + count a multiple
of 16, a short sequence first and a short one last.  (The sequence without a region keeps all its rows in the full-pass layout: see
modcr_hip.LiveRows.)"""
import numpy as np
import pytest
import torch

import helpers as H

gpu = pytest.mark.gpu

HID, HEADS, N_SEQ = 256, 4, 6
SHAPES = {"tile128": (24, 56), "tile192": (40, 100)}
SENTINEL = 1234.5      # exact in bf16


def region_counts(t, r):
    """short first, short last; R, 0, 1, R - 1 and T + 8 a multiple of 16 in between"""
    assert (t + 8) % 16 == 0
    return [1, r, 0, r - 1, 8, 1]


def host_batch(t, r, seed=5):
    """a synthetic batch of 2 examples x 3 choices = 6 sequences whose image masks carry region_counts(t, r)"""
    from Data import synthetic
    b = synthetic.make_batch(2, T=t, R=r, seed=seed, img_dim=70, min_text=t // 2, num_choices=3, vocab_size=400)
    for n, c in enumerate(region_counts(t, r)):
        b["input_mask"][n, t:] = 0
        b["input_mask"][n, t:t + c] = 1
        b["total_label"][n] = b["total_label"][n].clamp(max=max(c - 1, 0))
    return b


# ---- host tables (no GPU) ---------------------------------------------------------------------------------------------------------
def test_host_table_builder():
    import modcr_hip as mh
    t, r = 24, 56
    counts = region_counts(t, r)
    mask = torch.zeros(N_SEQ, t + r)
    mask[:, :10] = 1
    for n, c in enumerate(counts):
        mask[n, t:t + c] = 1
    live = mh.live_rows_from_mask(mask, t)
    assert live is not None and live.nreg.tolist() == counts and (live.n, live.t, live.r) == (N_SEQ, t, r)
    live.to(torch.device("cpu"))
    for lay, k in ((live.full, t), (live.img, 1)):
        s = k + r
        # (a [text | regions] sequence without a live region keeps every row: its padded text rows have all keys hidden under the
        # phase masks, and their uniform softmax runs over the padded regions too)
        ln = [k + (r if (c == 0 and k == t) else c) for c in counts]
        rs = np.concatenate([[0], np.cumsum(ln)])
        assert lay.seq_len == s and lay.capacity == N_SEQ * s and lay.m_live == rs[-1]
        assert lay.m_launch == min((rs[-1] + 255) // 256 * 256, N_SEQ * s)          # rounded to 256, capped at the capacity
        assert lay.row_start.dtype == torch.int32 and lay.row_start.tolist() == rs.tolist()
        rid = [n * s + j for n in range(N_SEQ) for j in range(ln[n])]
        assert lay.row_id.tolist() == rid + [-1] * (lay.m_launch - len(rid))
        assert lay.take[1].tolist() == rs[:-1].tolist()
        if k == t:
            assert lay.take[t].tolist() == [rs[n] + j for n in range(N_SEQ) for j in range(t)]
    # the pair: the full pass's live rows, then the image-only pass's; row_id = the index inside the padded pair buffer
    m1, m2, s1, s2 = live.full.m_live, live.img.m_live, t + r, 1 + r
    assert live.pair.m_live == m1 + m2 and live.pair.capacity == N_SEQ * (s1 + s2)
    assert live.pair.m_launch == min((m1 + m2 + 255) // 256 * 256, live.pair.capacity) and live.pair.m_launch % 256 == 0
    want = live.full.row_id[:m1].tolist() + [N_SEQ * s1 + v for v in live.img.row_id[:m2].tolist()]
    assert live.pair.row_id.tolist() == want + [-1] * (live.pair.m_launch - m1 - m2)
    assert live.pair.take["img"].tolist() == [m1 + v for v in live.img.row_start[:-1].tolist()]
    assert live.pair.take[t].tolist() == live.full.take[t].tolist()
    assert live.dead_rows == sum(r - c for c in counts if c) + sum(r - c for c in counts)
    # the region rows the region pipeline computes: those of the full pass's layout (all R slots where there is no live region)
    lr = [r if c == 0 else c for c in counts]
    rr = np.concatenate([[0], np.cumsum(lr)])
    assert live.reg.seq_len == r and live.reg.capacity == N_SEQ * r and live.reg.m_live == rr[-1]
    assert live.reg.m_launch == min((rr[-1] + 255) // 256 * 256, N_SEQ * r)
    assert live.reg.row_start.tolist() == rr.tolist()
    ids = [n * r + j for n in range(N_SEQ) for j in range(lr[n])]
    assert live.reg.row_id.tolist() == ids + [-1] * (live.reg.m_launch - len(ids))
    # nothing dead: M' = M
    full = mh.LiveRows([r] * 4, t, r).to(torch.device("cpu"))
    assert full.full.m_live == full.full.m_launch == full.full.capacity and full.pair.m_launch == full.pair.capacity
    assert full.full.row_id.tolist() == list(range(4 * (t + r)))
    # not in prefix form / dead [CLS] / a device-side or region-less mask: no tables
    bad = mask.clone()
    bad[2, t + 3] = 1
    assert mh.live_rows_from_mask(bad, t) is None
    bad = mask.clone()
    bad[1, t] = 0
    assert mh.live_rows_from_mask(bad, t) is None
    bad = mask.clone()
    bad[4, 0] = 0
    assert mh.live_rows_from_mask(bad, t) is None
    assert mh.live_rows_from_mask(mask[:, :t], t) is None
    with pytest.raises(ValueError):
        mh.LiveRows([r + 1], t, r)


def test_batch_to_device_attaches_the_tables_to_prefix_form_batches_only():
    from modeling import train_utils as tu
    b = host_batch(24, 56)
    moved = tu.batch_to_device(b, torch.device("cpu"))
    assert moved["live_rows"].nreg.tolist() == region_counts(24, 56) and moved["live_rows_tables"] is moved["live_rows"].blob
    assert tu.forward_inputs(moved)["live_rows"] is moved["live_rows"]
    b["input_mask"][3, 24 + 30] = 0               # a hole in the region part of a sequence with 55 regions
    moved = tu.batch_to_device(b, torch.device("cpu"))
    assert "live_rows" not in moved and "live_rows" not in tu.forward_inputs(moved)


def test_in_step_gemm_routes_are_the_padded_ones():
    """host only (modcr_linear_route launches nothing): at the headline shape -- 512 sequences, T = 80, R = 100, H = 768 -- the
    rounded live-row counts of the benchmark's batches take the GEMM routes of the padded counts, so the products stay bit-identical"""
    import modcr_hip as mh
    from Data import synthetic
    h, kp = 768, 2112

    def layer_routes(m):
        return [mh.linear_route((m, k), (n, k), bias=1, **kw) for k, n, kw in
                ((h, h, dict(out_dtype=mh.F16)), (h, 4 * h, dict(act=mh.ACT_GELU)), (4 * h, h, dict(out_dtype=mh.F16)))]
    launch = {1234: (102400, 71424), 1235: (103424, 71936)}
    for seed, (m_pair, m_seq) in launch.items():
        live = mh.live_rows_from_mask(synthetic.make_batch(128, seed=seed)["input_mask"], 80).to(torch.device("cpu"))
        assert (live.pair.capacity, live.full.capacity, live.reg.capacity) == (143872, 92160, 51200)
        assert (live.pair.m_launch, live.full.m_launch) == (m_pair, m_seq)
        assert layer_routes(m_pair) == layer_routes(143872) and layer_routes(m_seq) == layer_routes(92160)
        assert live.reg.m_launch % 256 == 0 and live.reg.m_launch < 0.65 * 51200
        # the region embedding (K = 2054 -> 2112: no persistent route) stays in the ring family.  Its tile size follows M, but the
        # family is ONE kernel template: every output element is one fp32 MFMA accumulator fed the same 16-wide K steps in the same
        # order whatever the tile (no split over K on the forward path), so the tile size changes no value
        rings = ("ring128", "ring192", "ring256")
        assert mh.linear_route((live.reg.m_launch, kp), (h, kp), bias=1, out_dtype=mh.F32).kernel in rings
        assert mh.linear_route((51200, kp), (h, kp), bias=1, out_dtype=mh.F32).kernel in rings


# ---- kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import modcr_hip as mh
    mh.lib()
    return torch.device("cuda")


def attn_inputs(t, r, dev, img_only=False):
    """(x [N,S,H] bf16, wqkv, bqkv, input_mask [N,S], chunk_mask [N,T,T], chunk_id [N,T], LiveLayout, LiveRows)"""
    import modcr_hip as mh
    from modeling import train_utils as tu
    b = host_batch(t, r)
    live = mh.live_rows_from_mask(b["input_mask"], t).to(dev)
    rs = np.random.RandomState(11)
    w = torch.from_numpy(rs.standard_normal((3 * HID, HID)).astype(np.float32) * 0.05).to(dev).to(torch.bfloat16)
    bias = torch.from_numpy(rs.standard_normal(3 * HID).astype(np.float32) * 0.1).to(dev)
    if img_only:
        mask = torch.cat([b["input_mask"][:, :1], b["input_mask"][:, t:]], 1).to(dev)
        lay = live.img
    else:
        mask, lay = b["input_mask"].to(dev), live.full
    s = mask.shape[1]
    x = torch.from_numpy(rs.standard_normal((N_SEQ, s, HID)).astype(np.float32)).to(dev).to(torch.bfloat16)
    cid = tu.pack_gather_index(b["gather_index"], t).to(dev)
    return x, w, bias, mask, b["chunk_attention_mask"].to(dev), cid, lay, live


def guarded(rows, h, dev, fill=SENTINEL, guard=8):
    """a [rows, h] bf16 view in the middle of a sentinel-filled allocation, and the allocation"""
    full = torch.full((rows + 2 * guard, h), fill, dtype=torch.bfloat16, device=dev)
    return full[guard:guard + rows], full


def live_equal(compact, padded, lay, n, s):
    """rows row_start[n] + j of `compact` == rows (n, j) of `padded` [N,S,H] for every live row, bit for bit"""
    rs = lay.row_start.tolist()
    for i in range(n):
        ln = rs[i + 1] - rs[i]
        if not torch.equal(compact[rs[i]:rs[i + 1]], padded[i, :ln]):
            return False
    return True


# (shape, KMODE): both tiles under the three production variants; the image-only pass [CLS | 100 regions] = 101 rows on the 128-token
# tile launches the key-mask variant only (its 57-row twin is the older kernel's: refused, see the next test)
ATTN_CASES = [(sh, km) for sh in ("tile128", "tile192") for km in (1, 2, 3)] + [("img101", 1)]


@gpu
@pytest.mark.parametrize("drop", [False, True], ids=["eval", "attn_dropout"])
@pytest.mark.parametrize("shape,kmode", ATTN_CASES, ids=["%s_kmode%d" % c for c in ATTN_CASES])
def test_attention_rows_entry_equals_the_padded_entry(dev, shape, kmode, drop):
    import modcr_hip as mh
    img_only = shape == "img101"
    t, r = SHAPES["tile192" if img_only else shape]
    x, w, bias, mask, cmask, cid, lay, live = attn_inputs(t, r, dev, img_only)
    n, s, h = x.shape
    route = mh.qkv_attn_route(n, s, 0, h, HEADS, dense=kmode >= 2, chunk_t=t if kmode == 3 else 0, align_t=t if kmode == 3 else 0,
                              attn_p=0.1 if drop else 0.0, flags=1 if (drop and kmode == 3) else 0, rows=True)
    assert route.rc == 0 and route.family == "tile4" and route.inst[:2] == (kmode, 128 if s <= 128 else 192), route
    kw = {}
    if kmode == 1:
        kw["key_mask"] = mask
    else:
        kw["mask_bits"] = mh.build_phase_mask(mask, cmask, 1 if kmode == 2 else 3)
    if kmode == 3:
        kw.update(chunk_id=cid, align_t=t)
    if drop:
        kw.update(attn_dropout=(0.1, 77, 4096), side_post_dropout=kmode == 3)
    amap_pad = torch.zeros(n, t, r, device=dev) if kmode == 3 else None
    ctx_pad, _ = mh.qkv_attn(x, w, bias, num_heads=HEADS, align_map=amap_pad, **kw)
    # live layout: compact x, context into a sentinel-filled buffer with guard rows on both sides
    xc = torch.zeros_like(x).view(n * s, h)
    mh.rows_take(x.view(n * s, h), lay.row_id, out=xc[:lay.m_launch])
    assert live_equal(xc, x, lay, n, s)
    ctx, ctx_alloc = guarded(n * s, h, dev)
    amap = torch.zeros(n, t, r, device=dev) if kmode == 3 else None
    out, probs = mh.qkv_attn(xc.view(n, s, h), w, bias, num_heads=HEADS, align_map=amap, out=ctx.view(n, s, h), row_start=lay.row_start, **kw)
    torch.cuda.synchronize()
    assert probs is None and out.data_ptr() == ctx.data_ptr()
    assert lay.m_live < n * s
    assert live_equal(ctx, ctx_pad, lay, n, s)
    assert bool((ctx[lay.m_live:] == SENTINEL).all()), "rows behind M' were written"
    assert bool((ctx_alloc[:8] == SENTINEL).all()) and bool((ctx_alloc[-8:] == SENTINEL).all()), "guard rows were written"
    if kmode == 3:
        assert torch.equal(amap, amap_pad)
        assert float(amap.abs().sum()) > 0


@gpu
def test_attention_rows_entry_refuses_before_launching(dev):
    import modcr_hip as mh
    lib = mh.lib()
    t, r = SHAPES["tile192"]
    x, w, bias, mask, cmask, cid, lay, live = attn_inputs(t, r, dev)
    n, s, h = x.shape
    ctx = torch.full_like(x, SENTINEL)
    st = mh._stream()

    def call(x_=x, w_=w, km=mask, bits=None, chunk=None, chunk_t=0, amap=None, align_t=0, rs=lay.row_start, n_=n, s_=s, h_=h, a_=HEADS,
             p=0.0, flags=0, dt=mh.BF16):
        return lib.modcr_qkv_attn_rows_fwd(mh._ptr(x_), mh._ptr(w_), mh._ptr(bias), mh._ptr(km), mh._ptr(bits), mh._ptr(chunk), chunk_t,
                                           mh._ptr(ctx), mh._ptr(amap), align_t, mh._ptr(rs), n_, s_, h_, a_, float(p), 0, 0, flags, dt, st)
    bits = mh.build_phase_mask(mask, cmask, 3)
    amap = torch.zeros(n, t, r, device=dev)
    cases = {
        "fp32": (dict(dt=mh.F32), -3),
        "above 192 keys (the 256-token tile)": (dict(s_=200, n_=4), -3),
        "above 256 keys (the streaming core)": (dict(s_=300, n_=2), -3),
        "at most 64 keys (the older tile kernel)": (dict(s_=57), -3),
        "odd head count (the older tile kernel)": (dict(h_=192, a_=3), -3),
        "chunk-mean queries without the align map (the generic variant)": (dict(bits=bits, chunk=cid, chunk_t=t), -3),
        "an align map without chunk ids (the generic variant)": (dict(bits=bits, amap=amap, align_t=t), -3),
        "no row_start": (dict(rs=None), -1),
        "no mask": (dict(km=None), -1),
        "unknown flags": (dict(flags=2), -1),
    }
    for what, (kw, rc) in cases.items():
        assert call(**kw) == rc, what
        assert lib.modcr_last_error(), what
    # what the entry has no argument for is refused by the route query the same way: prefix rows, probabilities, lse, q|k|v dump
    for kw in (dict(p=10), dict(probs=True), dict(lse=True), dict(lse=True, dump=True)):
        q = dict(n=n, s=s, p=0, h=h, a=HEADS, rows=True)
        q.update(kw)
        assert mh.qkv_attn_route(**q).rc == -3, kw
    with pytest.raises(ValueError):
        mh.qkv_attn(x, w, bias, key_mask=mask, num_heads=HEADS, row_start=lay.row_start, want_probs=True)
    torch.cuda.synchronize()
    assert bool((ctx == SENTINEL).all()) and float(amap.abs().sum()) == 0.0, "a refused call wrote"


@gpu
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["eval", "dropout"])
def test_linear_dropout_residual_ln_with_row_id(dev, p):
    import modcr_hip as mh
    t, r = SHAPES["tile128"]
    live = mh.LiveRows(region_counts(t, r), t, r).to(dev)
    lay = live.pair
    cap, m, k = lay.capacity, lay.m_launch, HID
    rs = np.random.RandomState(3)
    a = torch.from_numpy(rs.standard_normal((cap, k)).astype(np.float32)).to(dev).to(torch.bfloat16)
    res = torch.from_numpy(rs.standard_normal((cap, HID)).astype(np.float32)).to(dev).to(torch.bfloat16)
    w = torch.from_numpy(rs.standard_normal((HID, k)).astype(np.float32) * 0.05).to(dev).to(torch.bfloat16)
    b, g, be = (torch.from_numpy(rs.standard_normal(HID).astype(np.float32)).to(dev) for _ in range(3))
    seed, off = 99, 1 << 20
    assert mh.linear_route((cap, k), (HID, k), bias=1, out_dtype=mh.F16) == mh.linear_route((m, k), (HID, k), bias=1, out_dtype=mh.F16)
    y_pad = mh.linear_dropout_residual_ln(a, w, b, res, g, be, 1e-12, p, seed, off)
    ac, rc_ = mh.rows_take(a, lay.row_id), mh.rows_take(res, lay.row_id)
    out, alloc = guarded(m, HID, dev)
    mh.linear_dropout_residual_ln(ac, w, b, rc_, g, be, 1e-12, p, seed, off, out=out, row_id=lay.row_id)
    torch.cuda.synchronize()
    rid = lay.row_id[:lay.m_live].long()
    assert torch.equal(out[:lay.m_live], y_pad[rid])
    assert bool((alloc[:8] == SENTINEL).all()) and bool((alloc[-8:] == SENTINEL).all())
    # row_id = NULL is the entry it extends, bit for bit
    assert torch.equal(mh.linear_dropout_residual_ln(a, w, b, res, g, be, 1e-12, p, seed, off),
                       mh.linear_dropout_residual_ln(a, w, b, res, g, be, 1e-12, p, seed, off,
                                                     row_id=torch.arange(cap, dtype=torch.int32, device=dev)))


@gpu
def test_hidden_dropout_keep_mask_is_the_padded_buffers(dev):
    """x = 1 everywhere, no residual: the pre-LayerNorm rows are 0 or 1 / (1 - p), i.e. the keep decisions themselves"""
    import modcr_hip as mh
    t, r = SHAPES["tile128"]
    live = mh.LiveRows(region_counts(t, r), t, r).to(dev)
    lay = live.full
    m, h, p, seed, off = lay.m_launch, HID, 0.25, 12345, 4 * 777
    x = torch.ones(m, h, device=dev)
    g, be = torch.ones(h, device=dev), torch.zeros(h, device=dev)
    out = torch.empty(m, h, device=dev)
    pre = torch.empty(m, h, device=dev)
    rid = lay.row_id.clamp(min=0).contiguous()          # (the filler rows' entries only have to be valid counters)
    rc = mh.lib().modcr_dropout_residual_ln_rows_fwd(mh._ptr(x), mh.F32, None, 0, mh._ptr(g), mh._ptr(be), 1e-12, mh._ptr(out), mh.F32,
                                                     mh._ptr(pre), mh.F32, m, h, p, seed, off, mh._ptr(rid), mh._stream())
    assert rc == 0, mh.lib().modcr_last_error()
    keep = H.hidden_drop_keep(seed, off, lay.capacity * h, p).reshape(lay.capacity, h)
    got = (pre[:lay.m_live] != 0).cpu().numpy()
    assert np.array_equal(got, keep[lay.row_id[:lay.m_live].cpu().numpy()])
    assert 0.6 < got.mean() < 0.9


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_rows_take_compacts_and_gathers(dev, dtype):
    import modcr_hip as mh
    t, r = SHAPES["tile192"]
    live = mh.LiveRows(region_counts(t, r), t, r).to(dev)
    lay, s = live.full, t + r
    rs = np.random.RandomState(1)
    padded = torch.from_numpy(rs.standard_normal((N_SEQ, s, HID)).astype(np.float32)).to(dev).to(dtype)
    # padded -> compact: live rows equal, filler rows zero
    alloc = torch.full((lay.m_launch + 16, HID), SENTINEL, dtype=dtype, device=dev)
    compact = alloc[8:8 + lay.m_launch]
    mh.rows_take(padded.view(-1, HID), lay.row_id, out=compact)
    torch.cuda.synchronize()
    assert live_equal(compact, padded, lay, N_SEQ, s)
    assert bool((compact[lay.m_live:] == 0).all())
    assert bool((alloc[:8] == SENTINEL).all()) and bool((alloc[-8:] == SENTINEL).all())
    # compact -> dense [N, k, H]: k = T (the text rows) and k = 1 ([CLS])
    for k in (t, 1):
        got = mh.rows_take(compact, lay.take[k]).view(N_SEQ, k, HID)
        assert torch.equal(got, padded[:, :k])
    # an index outside the source gives a zero row
    idx = torch.tensor([0, -1, lay.m_launch, 3], dtype=torch.int32, device=dev)
    got = mh.rows_take(compact, idx)
    assert torch.equal(got[0], compact[0]) and torch.equal(got[3], compact[3]) and bool((got[1:3] == 0).all())


def embed_tables(dev, vocab=400, max_pos=64):
    rs = np.random.RandomState(21)
    f = lambda *sh: torch.from_numpy(rs.standard_normal(sh).astype(np.float32)).to(dev)
    return dict(word=f(vocab, HID), pos=f(max_pos, HID), typ=f(2, HID), gamma=f(HID), beta=f(HID))


@gpu
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["eval", "dropout"])
@pytest.mark.parametrize("img_only", [False, True], ids=["full", "img_only"])
@pytest.mark.parametrize("shape", ["tile128", "tile192"])
def test_embedding_passes_write_compact_rows(dev, shape, img_only, p):
    """modcr_embed_ln_dropout_rows_fwd + modcr_rows_place_dropout against the padded passes (embed_ln + rows_scatter_dropout): every
    live row equal bit for bit (same values, the dropout decisions of the padded position), filler rows zero, nothing else touched;
    region rows given padded [N R, H] and back to back (the live region pipeline's output)"""
    import modcr_hip as mh
    t, r = SHAPES[shape]
    b = host_batch(t, r)
    live = mh.live_rows_from_mask(b["input_mask"], t).to(dev)
    lay, k = (live.img, 1) if img_only else (live.full, t)
    s = k + r
    tb = embed_tables(dev)
    ids = b["input_ids"][:, :k].contiguous().to(dev)
    tts = None if img_only else b["token_type_ids"][:, :k].contiguous().to(dev)
    rs = np.random.RandomState(2)
    regions = torch.from_numpy(rs.standard_normal((N_SEQ * r, HID)).astype(np.float32)).to(dev).to(torch.bfloat16)
    drop = (p, 777, 4 * 1001) if p else None
    args = (tb["word"], tb["pos"], tb["typ"], tb["gamma"], tb["beta"], 1e-12)
    padded = torch.full((N_SEQ, s, HID), SENTINEL, dtype=torch.bfloat16, device=dev)
    mh.embed_ln(ids, tts, None, *args, padded, s, dropout=drop)
    mh.rows_scatter_dropout(regions, padded, k, drop)
    assert not bool((padded == SENTINEL).all(-1).any())
    if p:       # the dropout is live: some elements of the region rows are zeroed
        assert 0.02 < float((padded[:, k:] == 0).float().mean()) < 0.25
    regions_live = mh.rows_take(regions, live.reg.row_id)
    for src, start in ((regions, None), (regions_live, live.reg.row_start)):
        compact, alloc = guarded(lay.m_launch, HID, dev)
        mh.embed_ln_rows(ids, tts, None, *args, compact, s, lay.row_start, dropout=drop)
        mh.rows_place_dropout(src, compact, lay.row_id, r, s, k, drop, src_start=start)
        torch.cuda.synchronize()
        assert live_equal(compact, padded, lay, N_SEQ, s)
        assert bool((compact[lay.m_live:] == 0).all())
        assert bool((alloc[:8] == SENTINEL).all()) and bool((alloc[-8:] == SENTINEL).all())
    # without the filler rows (forward_pair places the next pass's rows right behind): rows from m_live on stay untouched
    compact, alloc = guarded(lay.m_launch, HID, dev)
    mh.embed_ln_rows(ids, tts, None, *args, compact, s, lay.row_start, dropout=drop)
    mh.rows_place_dropout(regions_live, compact[:lay.m_live], lay.row_id[:lay.m_live], r, s, k, drop, src_start=live.reg.row_start)
    torch.cuda.synchronize()
    assert live_equal(compact, padded, lay, N_SEQ, s) and bool((alloc[8 + lay.m_live:] == SENTINEL).all())
    # a table that points outside the buffer writes nothing
    out, alloc = guarded(8, HID, dev)
    bad = torch.tensor([lay.capacity, -k - 5] * N_SEQ, dtype=torch.int32, device=dev)[:N_SEQ].contiguous()
    mh.embed_ln_rows(ids, tts, None, *args, out, s, bad, dropout=drop)
    torch.cuda.synchronize()
    assert bool((alloc == SENTINEL).all())


@gpu
@pytest.mark.parametrize("shape", ["tile128", "tile192"])
def test_region_pipeline_over_live_regions(dev, shape):
    """cast -> region GEMM -> LayerNorm over the live region rows only: every row equals the padded pipeline's, bit for bit"""
    import modcr_hip as mh
    t, r = SHAPES[shape]
    d, kp = 70, 128
    live = mh.LiveRows(region_counts(t, r), t, r).to(dev)
    reg = live.reg
    assert reg.m_live < reg.m_launch < reg.capacity or reg.m_launch == reg.capacity
    rs = np.random.RandomState(8)
    feats = torch.from_numpy(rs.standard_normal((N_SEQ, r, d)).astype(np.float32)).to(dev)
    w = torch.from_numpy(rs.standard_normal((HID, kp)).astype(np.float32) * 0.1).to(dev).to(torch.bfloat16)
    w[:, d:] = 0
    b, g, be = (torch.from_numpy(rs.standard_normal(HID).astype(np.float32)).to(dev) for _ in range(3))
    assert mh.linear_route((reg.capacity, kp), (HID, kp), bias=1, out_dtype=mh.F32, dtype=mh.BF16) == \
        mh.linear_route((reg.m_launch, kp), (HID, kp), bias=1, out_dtype=mh.F32, dtype=mh.BF16)
    src_pad = mh.cast_pad(feats, kp, mh.BF16)
    src = mh.cast_pad_rows(feats, kp, reg.row_id)
    rid = reg.row_id[:reg.m_live].long()
    assert src.shape == (reg.m_launch, kp) and torch.equal(src[:reg.m_live], src_pad[rid]) and bool((src[reg.m_live:] == 0).all())
    assert bool((src[:, d:] == 0).all())
    rows_pad = mh.layernorm(mh.linear(src_pad, w, b, out_dtype=mh.F32), g, be, 1e-12, out_dtype=mh.BF16)
    rows = mh.layernorm(mh.linear(src, w, b, out_dtype=mh.F32), g, be, 1e-12, out_dtype=mh.BF16)
    torch.cuda.synchronize()
    assert torch.equal(rows[:reg.m_live], rows_pad[rid])
    # an index outside the source gives a zero row
    idx = torch.tensor([3, -1, N_SEQ * r, 0], dtype=torch.int32, device=dev)
    got = mh.cast_pad_rows(feats, kp, idx)
    assert torch.equal(got[0], src_pad[3]) and torch.equal(got[3], src_pad[0]) and bool((got[1:3] == 0).all())


# ---- model level --------------------------------------------------------------------------------------------------------------------
def small_model(dev, dropout, **cfg_kw):
    from modeling import train_utils as tu
    from modeling.modeling_ensemble import Abstract_Specific
    from modeling.modeling_transfomres import BertImgModel
    from modeling.modeling_vcr_chunkalign_v10 import ChunkAlign_CLS_enc4_align_ensemble, SeqBertImgModel
    from modeling.roberta_prefix import PrefixPoolerStandIn
    torch.manual_seed(3)
    kw = dict(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, hidden_size=HID, num_hidden_layers=4,
              num_attention_heads=HEADS, img_feature_dim=70, max_position_embeddings=64, add_residual=True, add_local_residual=True)
    kw.update(cfg_kw)
    calec = ChunkAlign_CLS_enc4_align_ensemble(BertImgModel(tu.oscar_config(400, "bf16", **kw)), SeqBertImgModel(tu.oscar_config(400, "bf16", **kw)), num_labels=3)
    calec.set_train_encoders(False)
    return Abstract_Specific(calec_model=calec, clip_model=None, roberta_model=PrefixPoolerStandIn(), num_labels=3).to(dev)


class RowsCalls(object):
    """counts the attention launches of a forward by layout"""

    def __init__(self, monkeypatch):
        import modcr_hip as mh
        self.live = self.padded = 0
        orig = mh.qkv_attn

        def counted(*a, **k):
            if k.get("row_start") is not None:
                self.live += 1
            else:
                self.padded += 1
            return orig(*a, **k)
        monkeypatch.setattr(mh, "qkv_attn", counted)

    def take(self):
        out = (self.live, self.padded)
        self.live = self.padded = 0
        return out


def run_step(model, batch, names, seed=4242):
    import modcr_hip as mh
    from modeling import train_utils as tu
    mh.DROPOUT.manual_seed(seed)
    pd = dict(model.named_parameters())
    for p in pd.values():
        p.grad = None
    loss, _, logits = model(**tu.forward_inputs(batch))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), logits.detach().clone(), {k: pd[k].grad.detach().clone() for k in names}


def assert_same_step(a, b):
    assert torch.equal(a[0], b[0]), (float(a[0]), float(b[0]))
    assert torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) > 10
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def gemm_routes_agree(m_padded, m_live):
    import modcr_hip as mh
    for (k, n, kw) in ((HID, HID, dict(out_dtype=mh.F16)), (HID, 4 * HID, dict(act=mh.ACT_GELU)), (4 * HID, HID, dict(out_dtype=mh.F16))):
        assert mh.linear_route((m_padded, k), (n, k), bias=1, **kw) == mh.linear_route((m_live, k), (n, k), bias=1, **kw), (m_padded, m_live, k, n)


@gpu
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("shape", ["tile128", "tile192"])
def test_model_step_equals_the_padded_route(dev, monkeypatch, shape, train):
    import modcr_hip as mh
    from modeling import modeling_transfomres as mt
    from modeling import train_utils as tu
    t, r = SHAPES[shape]
    monkeypatch.setattr(mt, "PACK_SHORT", 0)            # N = 6 sequences of 57 rows would be packed three to a tile
    model = small_model(dev, 0.1)
    model.train(train)
    names = tu.trainable_parameters(model)
    for k, p in model.named_parameters():
        p.requires_grad_(k in names)
    batch = tu.batch_to_device(host_batch(t, r), dev)
    live = batch["live_rows"]
    gemm_routes_agree(live.full.capacity, live.full.m_launch)
    gemm_routes_agree(live.pair.capacity, live.pair.m_launch)
    assert mh.linear_route((live.reg.capacity, 128), (HID, 128), bias=1, out_dtype=mh.F32, dtype=mh.BF16) == \
        mh.linear_route((live.reg.m_launch, 128), (HID, 128), bias=1, out_dtype=mh.F32, dtype=mh.BF16)      # the region embedding (70 -> 128 columns)
    calls = RowsCalls(monkeypatch)
    monkeypatch.setattr(mt, "LIVE_ROWS", False)
    off = run_step(model, batch, names)
    assert calls.take() == (0, 4 + 8)
    monkeypatch.setattr(mt, "LIVE_ROWS", True)
    on = run_step(model, batch, names)
    # seq_enc's four launches always; global_enc's pair when the image-only pass (1 + R rows) is on a tile the entry serves
    assert calls.take() == ((12, 0) if 1 + r > 64 else (4, 8))
    assert_same_step(on, off)


@gpu
def test_fallbacks_run_the_padded_route(dev, monkeypatch):
    import modcr_hip as mh
    from modeling import modeling_transfomres as mt
    from modeling import train_utils as tu
    t, r = SHAPES["tile192"]
    model = small_model(dev, 0.1)
    model.train()
    names = tu.trainable_parameters(model)
    for k, p in model.named_parameters():
        p.requires_grad_(k in names)
    hb = host_batch(t, r)
    batch = tu.batch_to_device(hb, dev)
    calls = RowsCalls(monkeypatch)
    monkeypatch.setattr(mt, "LIVE_ROWS", False)
    ref = run_step(model, batch, names)
    calls.take()
    monkeypatch.setattr(mt, "LIVE_ROWS", True)
    # a batch without the tables
    bare = {k: v for k, v in batch.items() if not k.startswith("live_rows")}
    assert_same_step(run_step(model, bare, names), ref)
    assert calls.take() == (0, 12)
    # tables made for another batch shape
    other = dict(batch, live_rows=mh.LiveRows(region_counts(t, r)[:4], t, r).to(dev))
    assert_same_step(run_step(model, other, names), ref)
    assert calls.take() == (0, 12)
    # a mask that is not in prefix form gets no tables, and runs as it did
    holed = dict(hb, input_mask=hb["input_mask"].clone())
    holed["input_mask"][1, t + 3] = 0
    hbatch = tu.batch_to_device(holed, dev)
    assert "live_rows" not in hbatch
    monkeypatch.setattr(mt, "LIVE_ROWS", False)
    href = run_step(model, hbatch, names)
    monkeypatch.setattr(mt, "LIVE_ROWS", True)
    calls.take()
    assert_same_step(run_step(model, hbatch, names), href)
    assert calls.take() == (0, 12)
    # config.modcr_last_layer_rows keeps its own (padded) route
    for enc in (model.calec.global_enc, model.calec.seq_enc):
        monkeypatch.setattr(enc.config, "modcr_last_layer_rows", True, raising=False)
    monkeypatch.setattr(mt, "LIVE_ROWS", False)
    lref = run_step(model, batch, names)
    monkeypatch.setattr(mt, "LIVE_ROWS", True)
    calls.take()
    assert_same_step(run_step(model, batch, names), lref)
    assert calls.take()[0] == 0
    for enc in (model.calec.global_enc, model.calec.seq_enc):
        monkeypatch.setattr(enc.config, "modcr_last_layer_rows", False, raising=False)
    # history states: the encoder class takes the padded route whatever it is handed
    genc = model.calec.global_enc
    hist = [torch.randn(N_SEQ, 4, HID, device=dev).to(torch.bfloat16) for _ in genc.encoder.layer]
    ids, km = batch["input_ids"], torch.cat([torch.ones(N_SEQ, 4, device=dev), batch["input_mask"][:, :t]], 1)
    with torch.no_grad():
        mh.DROPOUT.manual_seed(5)
        want = genc(ids, attention_mask=km, token_type_ids=batch["token_type_ids"], encoder_history_states=hist)[0]
        calls.take()
        mh.DROPOUT.manual_seed(5)
        got = genc(ids, attention_mask=km, token_type_ids=batch["token_type_ids"], encoder_history_states=hist, live_rows=batch["live_rows"])[0]
    assert torch.equal(got, want) and calls.take()[0] == 0
    # S <= 64: the older tile kernel, which has no live-row layout
    sb = tu.batch_to_device(_short_batch(), dev)
    assert "live_rows" in sb
    monkeypatch.setattr(mt, "LIVE_ROWS", False)
    sref = run_step(model, sb, names)
    monkeypatch.setattr(mt, "LIVE_ROWS", True)
    calls.take()
    assert_same_step(run_step(model, sb, names), sref)
    assert calls.take()[0] == 0


def _short_batch():
    """T = 24, R = 40: S = 64 keys"""
    from Data import synthetic
    return synthetic.make_batch(2, T=24, R=40, seed=8, img_dim=70, min_text=12, num_choices=3, vocab_size=400, min_regions=5)
