"""GPU parity of the five-product attention backward (csrc/attn_bwd.hip, modcr_qkv_attn_lse_bwd) -- autograd of
CaptionBertSelfAttention.forward (modeling_bert.py:34-75; v10:55-107) from the forward's row statistics.

Checkers:
  * the CPU oracle under torch autograd (oracle.self_attention; with attention dropout: the same formula with the mask
    restated on the host from the counter layout of csrc/attn_common.h) at small sizes -- every mask form, chunk-mean
    queries, both token tiles, S at and around the tile edges, padded key tails, a query row that sees nothing;
  * AT THE BENCHED SIZE (BASELINE config 3: N = 512 sequences, S = 180, H = 768, A = 12, 6 144 workgroups): the oracle's
    autograd on a strided subset of the sequences (dx) and a torch fp32 autograd evaluation on the device over all of them
    (dx of every sequence, dWqkv, dbqkv);
  * the older core (statistics recomputed, ctx = lse = None) on the same inputs: the two cores must agree with the reference
    to the same bound.
Tolerance: bf16 path, 2e-2 relative to max(1, max|reference|) (BASELINE.json north_star), written at each check.
"""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import modcr_oracle as O
from test_hip_attn_fullsize import bf16r, chunk_mean_device, drop_keep

pytestmark = pytest.mark.gpu

TOL_BF16 = 2e-2
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def mh():
    import __graft_entry__ as g  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import modcr_hip
    modcr_hip.lib()
    return modcr_hip


def check(got, ref, tol, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite"
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    H.report_use(what, err / scale, tol)
    assert err <= tol * scale, "%s: max|err| %.4g > %.1e * %.3g" % (what, err, tol, scale)
    rel = float((got - ref).norm() / max(1e-20, float(ref.norm())))
    return err, rel


def attention(x, w, b, a, add, cid=None, keep=None, p=0.0):
    """modeling_bert.py:46-72 (+ v10:66-78 chunk-mean queries, + nn.Dropout on the probabilities with a given keep mask) in
    torch, any device: returns (ctx [N,S,H], log2-domain row statistics [N,A,S])"""
    n, s, h = x.shape
    qkv = torch.nn.functional.linear(x, w, b)
    q, k, v = qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:]
    if cid is not None:
        q = chunk_mean_device(q, cid)
    sp = lambda t: t.view(n, s, a, 64).transpose(1, 2)
    sc = sp(q) @ sp(k).transpose(-1, -2) / 8.0 + add
    probs = torch.softmax(sc, -1)
    lse2 = torch.logsumexp(sc, -1) * LOG2E
    if keep is not None:
        probs = probs * keep / (1.0 - p)
    return (probs @ sp(v)).transpose(1, 2).reshape(n, s, h), lse2


def make_inputs(n, s, t, h, a, mask, chunk, seed):
    rs = np.random.RandomState(seed)
    sd = {}
    for nm in ("query", "key", "value"):
        H._lin(rs, sd, nm, h, h)
    sd = H.to_torch(sd)
    w = bf16r(torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0))
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0)
    x = bf16r(torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)))
    dctx = bf16r(torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)))
    valid = rs.randint(max(2, s // 3), s + 1, size=n)
    valid[0] = s
    km = torch.from_numpy((np.arange(s)[None, :] < valid[:, None]).astype(np.float32))
    dense = None
    if mask == "dense":
        d = (rs.uniform(size=(n, s, s)) < 0.6).astype(np.float32)
        d *= km.numpy()[:, None, :]
        d[:, np.arange(s), np.arange(s)] = 1
        d[n - 1, min(4, s - 1), :] = 0                      # a query row that sees nothing
        dense = torch.from_numpy(d)
    cid = None
    if chunk:
        cid = torch.full((n, t), -1, dtype=torch.int32)
        for i in range(n):
            ln = int(rs.randint(max(1, t // 2), max(2, t - 1)))
            ids, c = [], 0
            while len(ids) < ln:
                k = int(rs.choice([1, 2, 3, 4], p=[.5, .3, .15, .05]))
                ids += [c] * min(k, ln - len(ids))
                c += 1
            cid[i, 1:1 + ln] = torch.tensor(ids, dtype=torch.int32)
    return w, b, x, dctx, km, dense, cid


def run_hip(mh, w, b, x, dctx, km, dense, cid, a, drop, new_core=True, use_dump=False):
    dev = torch.device("cuda")
    n, s, h = x.shape
    xd, wd, bd = x.to(dev).bfloat16(), w.to(dev).bfloat16(), b.to(dev)
    bits = mh.pack_mask_bits(dense.to(dev)) if dense is not None else None
    kmd = km.to(dev) if dense is None else None
    cidd = cid.to(dev) if cid is not None else None
    lse = torch.full((n, a, s), float("nan"), device=dev) if new_core else None
    dump = torch.full((mh.qkv_dump_numel(n, s, a),), float("nan"), device=dev, dtype=torch.bfloat16) if use_dump else None
    ctx, _ = mh.qkv_attn(xd, wd, bd, key_mask=kmd, mask_bits=bits, chunk_id=cidd, num_heads=a, attn_dropout=drop, lse=lse, dump=dump)
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    dx = mh.qkv_attn_bwd(dctx.to(dev).bfloat16(), xd, wd, bd, dw, db, key_mask=kmd, mask_bits=bits, chunk_id=cidd, num_heads=a,
                         attn_dropout=drop, ctx=ctx if new_core else None, lse=lse, dump=dump)
    torch.cuda.synchronize()
    return ctx, lse, dx, dw, db


@pytest.mark.parametrize("s,t,mask,chunk,p", [
    (180, 80, "key", False, 0.0), (180, 80, "key", False, 0.2), (180, 80, "dense", True, 0.0), (180, 80, "dense", True, 0.25),
    (192, 90, "dense", False, 0.1), (129, 60, "key", False, 0.1), (161, 70, "dense", False, 0.0),
    (101, 1, "key", False, 0.1), (106, 50, "key", False, 0.0), (128, 40, "dense", True, 0.3), (65, 30, "dense", False, 0.0),
    (97, 30, "key", False, 0.0)])
def test_attn_bwd5_vs_oracle(mh, s, t, mask, chunk, p):
    """the five-product core against torch autograd of the reference formula on the CPU (the oracle's self_attention is held to
    the same formula below), and against the older core"""
    n, h, a = 3, 256, 4
    lp = 128 if s <= 128 else 192
    w, b, x, dctx, km, dense, cid = make_inputs(n, s, t, h, a, mask, chunk, 1000 + s + (7 if chunk else 0))
    seed, off = 20240 + s, 987654321012
    drop = (p, seed, off) if p > 0 else None
    keep = drop_keep(list(range(n)), a, s, lp, p, seed, off, "cpu") if p > 0 else None
    add = O.extend_mask(dense if dense is not None else km)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ctx_ref, lse_ref = attention(xr, wr, br, a, add, cid=cid.long() if cid is not None else None, keep=keep, p=p)
    (ctx_ref * dctx).sum().backward()
    if p == 0:      # the formula above IS the oracle's (oracle.self_attention, the restatement pinned by G1 / G2)
        sdo = {"query.weight": w[:h], "key.weight": w[h:2 * h], "value.weight": w[2 * h:], "query.bias": b[:h], "key.bias": b[h:2 * h],
               "value.bias": b[2 * h:]}
        gi = None
        if cid is not None:
            gi = [cid[i][cid[i] >= 0].long() for i in range(n)]
        ctx_o, _ = O.self_attention(x, add, sdo, "", a, gather_index=gi)
        assert float((ctx_o - ctx_ref).detach().abs().max()) < 1e-4
    ctx, lse, dx, dw, db = run_hip(mh, w, b, x, dctx, km, dense, cid, a, drop)
    check(ctx.float().cpu(), ctx_ref, TOL_BF16, "ctx")             # padded query rows included: the masks hide keys, not queries
    # row statistics: log2 sum exp2 of the scores the kernel saw (bf16 Q.K^T): absolute 3e-2 in log2 units
    rows = (km[:, None, :] > 0).expand(n, a, s)
    assert torch.isfinite(lse).all()
    assert float(((lse.cpu() - lse_ref.detach()).abs() * rows).max()) < 3e-2
    e = {}
    e["dx"] = check(dx, xr.grad, TOL_BF16, "dx")
    e["dw"] = check(dw, wr.grad, TOL_BF16, "dwqkv")
    kb = slice(h, 2 * h)           # the key-bias gradient is analytically zero: rounding noise of a sum over N S rows on both sides
    dbm, dbr = db.clone(), br.grad.clone()
    dbm[kb] = 0; dbr[kb] = 0
    check(dbm, dbr, TOL_BF16, "dbqkv")
    assert float(db[kb].abs().max()) <= TOL_BF16 * max(1.0, float(br.grad.abs().max())) * (n * s) ** 0.5 * 0.25
    H.report_use("dx rel L2", e["dx"][1], 2e-2, kind="relative L2"); H.report_use("dw rel L2", e["dw"][1], 2e-2, kind="relative L2")
    assert e["dx"][1] < 2e-2 and e["dw"][1] < 2e-2, e           # relative L2 as well
    # the second form (attn_bwd6_kernel) on the images the forward dumped: nothing recomputed
    _, _, dx_d, dw_d, db_d = run_hip(mh, w, b, x, dctx, km, dense, cid, a, drop, use_dump=True)
    e["dx6"] = check(dx_d, xr.grad, TOL_BF16, "dx (dump form)")
    e["dw6"] = check(dw_d, wr.grad, TOL_BF16, "dwqkv (dump form)")
    dbm6 = db_d.clone(); dbm6[kb] = 0
    check(dbm6, dbr, TOL_BF16, "dbqkv (dump form)")
    H.report_use("dx6 rel L2", e["dx6"][1], 2e-2, kind="relative L2"); H.report_use("dw6 rel L2", e["dw6"][1], 2e-2, kind="relative L2")
    assert e["dx6"][1] < 2e-2 and e["dw6"][1] < 2e-2, e
    # the older core (statistics recomputed) on the same inputs
    _, _, dx_o, dw_o, _ = run_hip(mh, w, b, x, dctx, km, dense, cid, a, drop, new_core=False)
    check(dx_o, xr.grad, TOL_BF16, "dx (older core)")
    check(dw_o, wr.grad, TOL_BF16, "dwqkv (older core)")


@pytest.mark.parametrize("s,t,mask,chunk,p", [(230, 194, "key", False, 0.1), (256, 128, "dense", True, 0.2), (193, 100, "dense", False, 0.1),
                                              (230, 194, "key", False, 0.0)])
def test_attn_bwd_on_the_256_token_tile_with_attention_dropout(mh, s, t, mask, chunk, p):
    """192 < S <= 256 (BASELINE config 5's S = 230 with trainable encoders, VERDICT r03 missing 3): the forward runs the 256-token
    tile kernel with its attention-probability dropout, the backward the exact core (csrc/attn_bwd_older.hip attn_bwd_f32_kernel), which
    regenerates the forward's mask from the counter layout of csrc/attn_common.h (LP = 256) -- against torch autograd of the
    reference formula with the mask restated on the host."""
    n, h, a = 2, 256, 4
    w, b, x, dctx, km, dense, cid = make_inputs(n, s, t, h, a, mask, chunk, 3000 + s)
    seed, off = 777 + s, 123456789012
    drop = (p, seed, off) if p > 0 else None
    keep = drop_keep(list(range(n)), a, s, 256, p, seed, off, "cpu") if p > 0 else None
    add = O.extend_mask(dense if dense is not None else km)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ctx_ref, _ = attention(xr, wr, br, a, add, cid=cid.long() if cid is not None else None, keep=keep, p=p)
    (ctx_ref * dctx).sum().backward()
    ctx, _, dx, dw, db = run_hip(mh, w, b, x, dctx, km, dense, cid, a, drop, new_core=False)
    check(ctx.float().cpu(), ctx_ref, TOL_BF16, "ctx (256-token tile, dropout)")
    e_dx = check(dx, xr.grad, TOL_BF16, "dx (256-token tile)")
    e_dw = check(dw, wr.grad, TOL_BF16, "dwqkv (256-token tile)")
    kb = slice(h, 2 * h)
    dbm, dbr = db.clone(), br.grad.clone()
    dbm[kb] = 0; dbr[kb] = 0
    check(dbm, dbr, TOL_BF16, "dbqkv (256-token tile)")
    assert e_dx[1] < 2e-2 and e_dw[1] < 2e-2, (e_dx, e_dw)


@pytest.mark.parametrize("use_dump", [True, False])
@pytest.mark.parametrize("mask,p", [("key", 0.1), ("dense", 0.0)])
def test_attn_bwd5_full_size(mh, mask, p, use_dump):
    """BASELINE config 3's call: N = 512 sequences of S = 180, H = 768, 12 heads (6 144 workgroups, 24 per CU)."""
    n, s, t, h, a = 512, 180, 80, 768, 12
    dev = torch.device("cuda")
    w, b, x, dctx, km, dense, cid = make_inputs(n, s, t, h, a, mask, mask == "dense", 4242)
    seed, off = 99, 123456789
    drop = (p, seed, off) if p > 0 else None
    ctx, lse, dx, dw, db = run_hip(mh, w, b, x, dctx, km, dense, cid, a, drop, use_dump=use_dump)
    assert torch.isfinite(dx.float()).all() and torch.isfinite(dw).all()
    # checker 1: torch fp32 autograd on the device, all sequences, in chunks
    wd = w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True)
    dx_ref = torch.empty(n, s, h, device=dev)
    chunk = 32
    for i0 in range(0, n, chunk):
        sl = slice(i0, i0 + chunk)
        xs = x[sl].to(dev).requires_grad_(True)
        add = O.extend_mask((dense if dense is not None else km)[sl]).to(dev)
        keep = drop_keep(list(range(i0, i0 + chunk)), a, s, 192, p, seed, off, dev) if p > 0 else None
        c, _ = attention(xs, wd, bd, a, add, cid=cid[sl].to(dev).long() if cid is not None else None, keep=keep, p=p)
        (c * dctx[sl].to(dev)).sum().backward()
        dx_ref[sl] = xs.grad
    e_dx = check(dx, dx_ref, TOL_BF16, "dx (device reference, all sequences)")
    e_dw = check(dw, wd.grad, TOL_BF16, "dwqkv (device reference)")
    H.report_use("dx rel L2", e_dx[1], 2e-2, kind="relative L2"); H.report_use("dw rel L2", e_dw[1], 2e-2, kind="relative L2")
    assert e_dx[1] < 2e-2 and e_dw[1] < 2e-2, (e_dx, e_dw)
    dbm, dbr = db.clone(), bd.grad.clone()
    dbm[h:2 * h] = 0; dbr[h:2 * h] = 0
    check(dbm, dbr, TOL_BF16, "dbqkv (device reference)")
    # checker 2: the CPU oracle's autograd on a strided subset (dropout off: the oracle has no dropout mask input)
    if p == 0:
        ids = list(range(0, n, 37))[:12] + [n - 1]
        sdo = {"query.weight": w[:h], "key.weight": w[h:2 * h], "value.weight": w[2 * h:], "query.bias": b[:h], "key.bias": b[h:2 * h],
               "value.bias": b[2 * h:]}
        xs = x[ids].clone().requires_grad_(True)
        gi = [cid[i][cid[i] >= 0].long() for i in ids] if cid is not None else None
        c, _ = O.self_attention(xs, O.extend_mask((dense if dense is not None else km)[ids]), sdo, "", a, gather_index=gi)
        (c * dctx[ids]).sum().backward()
        check(dx[ids], xs.grad, TOL_BF16, "dx (oracle, strided subset)")


@pytest.mark.parametrize("s,t,mask,chunk", [(180, 80, "key", False), (180, 80, "dense", True), (101, 40, "key", False), (128, 60, "dense", True)])
def test_forward_dump_holds_the_projections(mh, s, t, mask, chunk):
    """modcr_qkv_attn_lse_fwd's qkv_dump: the Q | K | V images the forward held in LDS, as rows [N][A][3][LP][64] -- Q scaled by
    log2e / 8 and chunk-averaged (v10:66-78), K and V as projected (modeling_bert.py:36-44); rows beyond S are padding."""
    n, h, a = 3, 256, 4
    lp = 128 if s <= 128 else 192
    w, b, x, dctx, km, dense, cid = make_inputs(n, s, t, h, a, mask, chunk, 77 + s)
    dev = torch.device("cuda")
    lse = torch.empty(n, a, s, device=dev)
    dump = torch.full((mh.qkv_dump_numel(n, s, a),), float("nan"), device=dev, dtype=torch.bfloat16)
    bits = mh.pack_mask_bits(dense.to(dev)) if dense is not None else None
    ctx, _ = mh.qkv_attn(x.to(dev).bfloat16(), w.to(dev).bfloat16(), b.to(dev), key_mask=km.to(dev) if dense is None else None, mask_bits=bits,
                         chunk_id=cid.to(dev) if cid is not None else None, num_heads=a, lse=lse, dump=dump)
    ctx0, _ = mh.qkv_attn(x.to(dev).bfloat16(), w.to(dev).bfloat16(), b.to(dev), key_mask=km.to(dev) if dense is None else None, mask_bits=bits,
                          chunk_id=cid.to(dev) if cid is not None else None, num_heads=a)
    assert torch.equal(ctx, ctx0)                               # the side outputs do not touch the context rows
    d = dump.view(n, a, 3, lp, 64)[:, :, :, :s].float().cpu()
    qkv = torch.nn.functional.linear(x, w, b)
    q, k, v = qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:]
    if cid is not None:
        q = chunk_mean_device(q, cid.long())
    sp = lambda z: z.view(n, s, a, 64).transpose(1, 2)
    check(d[:, :, 0] / (LOG2E / 8.0), sp(q), TOL_BF16, "dumped Q")
    check(d[:, :, 1], sp(k), TOL_BF16, "dumped K")
    check(d[:, :, 2], sp(v), TOL_BF16, "dumped V")


@pytest.mark.parametrize("with_ctx,t,r,p", [(True, 80, 100, 0.0), (False, 80, 100, 0.0), (True, 80, 100, 0.2), (True, 33, 70, 0.0), (True, 60, 68, 0.1)])
def test_attn_bwd6_align_map_gradient(mh, with_ctx, t, r, p):
    """the align map's gradient (v10:1067-1073: d_align on the head-summed text -> region probabilities) through the dump form:
    attn_dalign_delta_kernel + attn_bwd6_kernel<DALIGN> against autograd of the reference formula; dense mask + chunk-mean
    queries as in seq_enc's layers 9-11, with and without attention dropout (the map sums the UNMASKED probabilities)."""
    n, h, a = 3, 256, 4
    s = t + r
    lp = 128 if s <= 128 else 192
    w, b, x, dctx, km, dense, cid = make_inputs(n, s, t, h, a, "dense", True, 500 + t)
    if not with_ctx:
        dctx = torch.zeros_like(dctx)
    rs = np.random.RandomState(t)
    d_align = torch.from_numpy(rs.standard_normal((n, t, r)).astype(np.float32))
    seed, off = 31 + t, 10007
    drop = (p, seed, off) if p > 0 else None
    keep = drop_keep(list(range(n)), a, s, lp, p, seed, off, "cpu") if p > 0 else None
    add = O.extend_mask(dense)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    qkv = torch.nn.functional.linear(xr, wr, br)
    q, k, v = qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:]
    q = chunk_mean_device(q, cid.long())
    sp = lambda z: z.view(n, s, a, 64).transpose(1, 2)
    probs = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 8.0 + add, -1)
    amap = probs.sum(1)[:, :t, t:]
    pm = probs * keep / (1.0 - p) if keep is not None else probs
    ctx_ref = (pm @ sp(v)).transpose(1, 2).reshape(n, s, h)
    ((ctx_ref * dctx).sum() + (amap * d_align).sum()).backward()
    dev = torch.device("cuda")
    xd, wd, bd = x.to(dev).bfloat16(), w.to(dev).bfloat16(), b.to(dev)
    bits = mh.pack_mask_bits(dense.to(dev))
    lse = torch.empty(n, a, s, device=dev)
    dump = torch.empty(mh.qkv_dump_numel(n, s, a), device=dev, dtype=torch.bfloat16)
    amap_hip = torch.zeros(n, t, r, device=dev)
    ctx, _ = mh.qkv_attn(xd, wd, bd, mask_bits=bits, chunk_id=cid.to(dev), num_heads=a, attn_dropout=drop, lse=lse, dump=dump,
                         align_map=amap_hip, align_t=t)
    check(amap_hip, amap, TOL_BF16, "align map")
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    dx = mh.qkv_attn_bwd(dctx.to(dev).bfloat16(), xd, wd, bd, dw, db, mask_bits=bits, chunk_id=cid.to(dev), num_heads=a, attn_dropout=drop,
                         d_align=d_align.to(dev), align_t=t, ctx=ctx, lse=lse, dump=dump)
    e_dx = check(dx, xr.grad, TOL_BF16, "dx")
    e_dw = check(dw, wr.grad, TOL_BF16, "dwqkv")
    H.report_use("dx rel L2", e_dx[1], 3e-2, kind="relative L2"); H.report_use("dw rel L2", e_dw[1], 3e-2, kind="relative L2")
    assert e_dx[1] <= 3e-2 and e_dw[1] <= 3e-2, (e_dx, e_dw)       # relative L2 (the bound of test_attn_bwd_align_map_gradient)


def test_attn_bwd6_launches_are_reproducible(mh):
    """attn_bwd6_kernel hands blocks between loader and compute waves through LDS with ONE barrier per block and keeps prefetches in
    flight across it: a protocol error would show as launches that differ.  60 launches at the bench size (24 tiles per persistent
    workgroup), caches flushed in between, dx / dW compared bit for bit with the first (every sum in the kernel has a fixed order;
    the weight-gradient GEMM behind it is deterministic too)."""
    n, s, t, h, a = 512, 180, 80, 768, 12
    dev = torch.device("cuda")
    w, b, x, dctx, km, dense, cid = make_inputs(n, s, t, h, a, "dense", True, 4243)
    xd, wd, bd = x.to(dev).bfloat16(), w.to(dev).bfloat16(), b.to(dev)
    bits, cidd = mh.pack_mask_bits(dense.to(dev)), cid.to(dev)
    drop = (0.1, 5, 77)
    lse = torch.empty(n, a, s, device=dev)
    dump = torch.empty(mh.qkv_dump_numel(n, s, a), device=dev, dtype=torch.bfloat16)
    ctx, _ = mh.qkv_attn(xd, wd, bd, mask_bits=bits, chunk_id=cidd, num_heads=a, attn_dropout=drop, lse=lse, dump=dump)
    dcd = dctx.to(dev).bfloat16()
    flush = torch.empty(300 << 20, dtype=torch.uint8, device=dev)
    first = None
    for i in range(60):
        flush.fill_(i & 0xff)
        dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
        dx = mh.qkv_attn_bwd(dcd, xd, wd, bd, dw, db, mask_bits=bits, chunk_id=cidd, num_heads=a, attn_dropout=drop, ctx=ctx, lse=lse, dump=dump)
        if first is None:
            first = (dx.clone(), dw.clone())
            assert torch.isfinite(first[0].float()).all() and torch.isfinite(first[1]).all()
        else:
            assert torch.equal(dx, first[0]), "launch %d: dx differs in %d elements" % (i, int((dx != first[0]).sum()))
            assert torch.equal(dw, first[1]), "launch %d: dwqkv differs" % i
