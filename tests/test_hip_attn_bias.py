"""GPU tests of the attention forward with an additive float mask / bias and a head mask (modcr_qkv_attn_bias_fwd: the bias
variant of the streaming core in csrc/attn_long.hip, behind modcr_hip.qkv_attn(attn_bias=, head_mask=) and the reference-signature
forward()s of the attention modules), P + S <= 512, bf16 and fp32, against the float64 oracle.

Reference: oracle.self_attention adds any broadcastable mask; the head mask is applied here as a per-head scale of the oracle's
probabilities and of the matching 64 context columns.  A query row whose every key is -inf leaves with context 0 and probabilities
0 (the reference's softmax gives NaN there: the one deliberate difference, include/modcr_hip.h).

Bounds: max|got - ref| <= bound x max(1, max|ref|); bf16 2e-2 and fp32 1e-3 (the repository's contract, tests/test_hip_attn_long.py),
the align map 1e-2 / 2e-3 as there.  One encoder layer and the 3-layer encoder in bf16: 2e-2 x 2 -- the attention's 2e-2 is followed
by two (six) more blocks that store bf16 rows, each renormalised by a LayerNorm; tests/test_hip_attn_long.py takes 2 x 2e-2 for one
bf16 layer and 3 x 2e-2 for twelve.  fp32 stays at 1e-3 at every depth, as there."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from oracle import modcr_oracle as O
from test_hip_attn_long import call, check, inputs, seq_batch, small_config, weights

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-3, torch.bfloat16: 2e-2}
ALIGN_TOL = {torch.float32: 2e-3, torch.bfloat16: 1e-2}
DT = [torch.bfloat16, torch.float32]
NEG_INF = float("-inf")

# (n, s, p, h, a): a single partial tile; L % 4 != 0 (unaligned bias rows); prefix rows, L = 190; the first key of the fifth tile;
# an odd head count with a prefix above 256 keys; the limit
SHAPES = [(2, 37, 0, 128, 2), (3, 101, 0, 128, 2), (2, 180, 10, 128, 2), (2, 257, 0, 128, 2), (2, 300, 10, 192, 3), (1, 512, 0, 128, 2)]
PROBS_AT = {(3, 101, 0, 128, 2), (2, 300, 10, 192, 3)}


@pytest.fixture(scope="module")
def mh():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import modcr_hip
    modcr_hip.lib()
    return modcr_hip


@functools.lru_cache(maxsize=None)
def case(n, s, p, h, a, dtype):
    """weights, rows and the float64 V of one shape, shared by every test on it (read-only)"""
    rs = np.random.RandomState(1000 * n + s + 7 * p + h)
    sd, sd64 = weights(rs, h, dtype)
    x, hist = inputs(rs, n, s, p, h, dtype)
    xs = x if hist is None else torch.cat([hist, x], 1)
    v = torch.nn.functional.linear(xs.double(), sd64["value.weight"], sd64["value.bias"]).view(n, p + s, a, 64).transpose(1, 2)
    return sd, sd64, x, hist, v


def soft_bias(rs, shape):
    """2 x randn with ~10 % of the entries -10000 and ~10 % -inf; key 0 of every row finite, so that no row is all -inf"""
    b = 2.0 * rs.standard_normal(shape).astype(np.float32)
    u = rs.uniform(size=shape)
    b[u < 0.1] = -10000.0
    b[(u >= 0.1) & (u < 0.2)] = NEG_INF
    b[..., 0] = rs.standard_normal(shape[:-1]).astype(np.float32)
    return torch.from_numpy(b)


def oracle(c, a, bias, hm=None, gi=None):
    """float64 (ctx, probs) with the head mask [A] / [N, A] applied to the probabilities and the context columns"""
    sd, sd64, x, hist, v = c
    n, s, h = x.shape
    add = torch.zeros(1, 1, 1, 1, dtype=torch.float64) if bias is None else bias.double()
    ctx, probs = O.self_attention(x.double(), add, sd64, "", a, history_state=None if hist is None else hist.double(), gather_index=gi)
    if hm is not None:
        hm = hm.double().reshape(-1, a)
        probs = probs * hm[:, :, None, None]
        ctx = (ctx.view(n, s, a, 64) * hm[:, None, :, None]).reshape(n, s, h)
    return ctx, probs


def run(mh, dtype, c, a, bias=None, hm=None, cid=None, align_t=0, want_probs=False, drop=None, post=False, **kw):
    """qkv_attn on the GPU; `bias` is handed over as it is when it already lives there (views keep their strides)"""
    sd, _, x, hist, _ = c
    w = torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0).to(dtype).cuda()
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0).cuda()
    n, s, _ = x.shape
    amap = torch.zeros(n, align_t, s - align_t, device="cuda") if align_t else None
    ctx, probs = mh.qkv_attn(x.to(dtype).cuda(), w, b, hist=None if hist is None else hist.to(dtype).cuda(),
                             chunk_id=None if cid is None else cid.cuda(), want_probs=want_probs, align_map=amap, align_t=align_t,
                             num_heads=a, attn_dropout=drop, side_post_dropout=post,
                             attn_bias=None if bias is None else bias.cuda(), head_mask=None if hm is None else hm.cuda(), **kw)
    return ctx, probs, amap


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,s,p,h,a", SHAPES)
def test_soft_bias_in_every_broadcast_form(mh, dtype, n, s, p, h, a):
    c = case(n, s, p, h, a, dtype)
    l = p + s
    rs = np.random.RandomState(s + l)
    want = (n, s, p, h, a) in PROBS_AT
    forms = {"[N,1,1,L]": (n, 1, 1, l), "[N,1,S,L]": (n, 1, s, l), "[1,A,S,L]": (1, a, s, l), "[N,A,S,L]": (n, a, s, l)}
    for name, shape in forms.items():
        bias = soft_bias(rs, shape)
        ref_ctx, ref_p = oracle(c, a, bias)
        ctx, probs, _ = run(mh, dtype, c, a, bias=bias, want_probs=want)
        check(ctx, ref_ctx, TOL[dtype], "ctx " + name)
        if want:
            check(probs, ref_p, TOL[dtype], "probs " + name)
            if dtype == torch.float32:
                assert (probs.double().sum(-1) - 1).abs().max().item() <= 1e-5, name
    # an expand()ed, non-contiguous view: rows of a wider tensor (row stride L + 3), broadcast over the heads by stride 0
    wide = soft_bias(rs, (n, 1, s, l + 3))
    view = wide.cuda()[..., :l].expand(n, a, s, l)
    assert not view.is_contiguous() and view.stride(1) == 0 and view.stride(2) == l + 3
    ref_ctx, ref_p = oracle(c, a, wide[..., :l])
    ctx, probs, _ = run(mh, dtype, c, a, bias=view, want_probs=want)
    check(ctx, ref_ctx, TOL[dtype], "ctx expand()ed view")
    if want:
        check(probs, ref_p, TOL[dtype], "probs expand()ed view")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,s,p,h,a", [(3, 180, 10, 128, 2), (3, 300, 0, 128, 2)])
def test_binary_masks_through_the_general_route(mh, dtype, n, s, p, h, a):
    """a 0 / -10000 key mask (sequence 1 masks every key: the uniform softmax) and a dense mask as the bias, against the oracle
    and against the binary route of the same call"""
    c = case(n, s, p, h, a, dtype)
    sd, _, x, hist, _ = c
    l = p + s
    rs = np.random.RandomState(l)
    km = (np.arange(l)[None, :] < rs.randint(l // 2, l + 1, size=n)[:, None]).astype(np.float32)
    km[1] = 0
    dm = (rs.uniform(size=(n, s, l)) < 0.7).astype(np.float32)
    dm[0, 3, :] = 0
    for name, m01, kw in (("key mask", torch.from_numpy(km), "key_mask"), ("dense mask", torch.from_numpy(dm), "dense")):
        add = O.extend_mask(m01.double())
        ref_ctx, ref_p = oracle(c, a, add)
        ctx, probs, _ = run(mh, dtype, c, a, bias=add.float(), want_probs=True)
        check(ctx, ref_ctx, TOL[dtype], "ctx, %s as bias" % name)
        check(probs, ref_p, TOL[dtype], "probs, %s as bias" % name)
        ctx_b, probs_b, _ = call(mh, dtype, x, sd, a, hist=hist, want_probs=True, **{kw: m01})
        check(ctx, ctx_b.float(), TOL[torch.bfloat16], "ctx vs the binary route, " + name)
        check(probs, probs_b, TOL[torch.bfloat16], "probs vs the binary route, " + name)


@pytest.mark.parametrize("dtype", DT)
def test_row_of_minus_infinity_everywhere(mh, dtype):
    n, s, p, h, a = 3, 101, 0, 128, 2
    c = case(n, s, p, h, a, dtype)
    bias = soft_bias(np.random.RandomState(5), (n, a, s, s))
    bias[1, 0, 5, :] = NEG_INF
    bias[2, :, 70, :] = NEG_INF
    ctx, probs, _ = run(mh, dtype, c, a, bias=bias, want_probs=True)
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(probs).all()
    assert (probs[1, 0, 5] == 0).all() and (ctx[1, 5, :64] == 0).all()
    assert (probs[2, :, 70] == 0).all() and (ctx[2, 70] == 0).all()
    fin = bias.clone()                                      # the oracle on a finite stand-in for the two rows, then zeroed as specified
    fin[1, 0, 5, :] = 0
    fin[2, :, 70, :] = 0
    ref_ctx, ref_p = oracle(c, a, fin)
    ref_p[1, 0, 5] = 0
    ref_p[2, :, 70] = 0
    ref_ctx[1, 5, :64] = 0
    ref_ctx[2, 70] = 0
    check(ctx, ref_ctx, TOL[dtype], "ctx around all -inf rows")
    check(probs, ref_p, TOL[dtype], "probs around all -inf rows")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("with_bias", [False, True])
def test_head_mask(mh, dtype, with_bias):
    n, s, p, h, a = 3, 101, 0, 128, 2
    t = 60
    c = case(n, s, p, h, a, dtype)
    rs = np.random.RandomState(11 + with_bias)
    bias = soft_bias(rs, (n, 1, s, s)) if with_bias else None
    masks = {"[A]": torch.tensor([0.0, 0.5]), "[N,A]": torch.from_numpy(rs.uniform(size=(n, a)).astype(np.float32)),
             "[N,A,1,1]": torch.from_numpy(rs.uniform(size=(n, a, 1, 1)).astype(np.float32))}
    for name, hm in masks.items():
        ref_ctx, ref_p = oracle(c, a, bias, hm)
        ctx, probs, amap = run(mh, dtype, c, a, bias=bias, hm=hm, want_probs=True, align_t=t)
        check(ctx, ref_ctx, TOL[dtype], "ctx, head mask " + name)
        check(probs, ref_p, TOL[dtype], "probs, head mask " + name)
        check(amap, ref_p.sum(1)[:, :t, t:], ALIGN_TOL[dtype], "align map, head mask " + name)
        if name == "[A]":
            assert (ctx[:, :, :64] == 0).all() and (probs[:, 0] == 0).all()


@pytest.mark.parametrize("dtype", DT)
def test_chunk_mean_queries_and_align_map(mh, dtype):
    """a seq_enc-shaped call (T = 60, R = 41): the phase-3 mask as an additive bias with a soft term on top, chunk-mean queries, align map"""
    n, t, r, h, a = 3, 60, 41, 128, 2
    c = case(n, t + r, 0, h, a, dtype)
    rs = np.random.RandomState(60)
    im, cm, gi, cid = seq_batch(rs, n, t, r)
    add = O.seq_phase_mask(im.double(), cm.double(), t, r, 3).float() + torch.from_numpy(rs.standard_normal((n, 1, t + r, t + r)).astype(np.float32))
    ref_ctx, ref_p = oracle(c, a, add, gi=gi)
    ctx, probs, amap = run(mh, dtype, c, a, bias=add, cid=cid, align_t=t, want_probs=True)
    check(ctx, ref_ctx, TOL[dtype], "phase-3 ctx")
    check(probs, ref_p, TOL[dtype], "phase-3 probs")
    check(amap, ref_p.sum(1)[:, :t, t:], ALIGN_TOL[dtype], "phase-3 align map")
    ctx2, _, amap2 = run(mh, dtype, c, a, bias=add, cid=cid, align_t=t)
    check(ctx2, ref_ctx, TOL[dtype], "phase-3 ctx (align map only)")
    check(amap2, ref_p.sum(1)[:, :t, t:], ALIGN_TOL[dtype], "phase-3 align map (without probs)")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,s,p,h,a", [(2, 101, 0, 128, 2), (2, 180, 10, 128, 2)])
def test_attention_dropout_up_to_256_keys(mh, dtype, n, s, p, h, a):
    c = case(n, s, p, h, a, dtype)
    sd, _, x, hist, v = c
    l = p + s
    pd, seed, off = 0.2, 77, 5 << 32
    rs = np.random.RandomState(l + 1)
    bias = soft_bias(rs, (n, 1, s, l))
    hm = torch.tensor([1.0, 0.5])
    keep = H.attn_drop_keep_torch(range(n), a, s, pd, seed, off, "cpu", keys=l).double()
    _, ref_p = oracle(c, a, bias)                           # un-dropped, without the head mask
    pdrop = ref_p * keep / (1 - pd) * hm.double()[None, :, None, None]
    ref_ctx = (pdrop @ v).transpose(1, 2).reshape(n, s, h)
    ctx, _, _ = run(mh, dtype, c, a, bias=bias, hm=hm, drop=(pd, seed, off))
    check(ctx, ref_ctx, TOL[dtype], "ctx under dropout")
    ctx2, probs, _ = run(mh, dtype, c, a, bias=bias, hm=hm, drop=(pd, seed, off), want_probs=True, post=True)
    check(ctx2, ref_ctx, TOL[dtype], "ctx under dropout (with probs)")
    assert (probs.cpu()[keep == 0] == 0).all(), "a dropped probability is exactly 0"
    check(probs, pdrop, TOL[dtype], "post-dropout probs")
    _, probs_u, _ = run(mh, dtype, c, a, bias=bias, hm=hm, drop=(pd, seed, off), want_probs=True)
    check(probs_u, ref_p * hm.double()[None, :, None, None], TOL[dtype], "un-dropped probs under dropout")
    # a 0 / -10000 bias: the mask bits of the binary route for the same (seed, offset)
    km = torch.ones(n, l)
    km[1, l - 30:] = 0
    ctx_g, _, _ = run(mh, dtype, c, a, bias=O.extend_mask(km), drop=(pd, seed, off))
    w = torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0).to(dtype).cuda()
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0).cuda()
    ctx_b, _ = mh.qkv_attn(x.to(dtype).cuda(), w, b, key_mask=km.cuda(), hist=None if hist is None else hist.to(dtype).cuda(),
                           num_heads=a, attn_dropout=(pd, seed, off))
    check(ctx_g, ctx_b.float(), TOL[torch.bfloat16], "ctx under dropout vs the binary route")


@pytest.mark.parametrize("dtype", DT)
def test_deterministic(mh, dtype):
    n, s, p, h, a = 2, 300, 10, 192, 3
    c = case(n, s, p, h, a, dtype)
    bias = soft_bias(np.random.RandomState(2), (n, a, s, p + s))
    hm = torch.tensor([0.25, 1.0, 0.5])
    c1, p1, _ = run(mh, dtype, c, a, bias=bias, hm=hm, want_probs=True)
    c2, p2, _ = run(mh, dtype, c, a, bias=bias, hm=hm, want_probs=True)
    assert torch.equal(c1, c2) and torch.equal(p1, p2)


def test_refusals(mh):
    dtype, h, a = torch.bfloat16, 128, 2
    rs = np.random.RandomState(4)
    sd, _ = weights(rs, h, dtype)
    x, hist = inputs(rs, 1, 503, 10, h, dtype)
    with pytest.raises(ValueError, match="512"):
        run(mh, dtype, (sd, None, x, hist, None), a, bias=torch.zeros(1, 1, 1, 513))
    c = (sd, None, x[:, :300].contiguous(), None, None)
    with pytest.raises((ValueError, mh.ModcrHipError), match="256"):
        run(mh, dtype, c, a, bias=torch.zeros(1, 1, 1, 300), drop=(0.1, 1, 2))
    with pytest.raises(ValueError, match="key_mask"):
        run(mh, dtype, c, a, bias=torch.zeros(1, 1, 1, 300), key_mask=torch.ones(1, 300).cuda())
    with pytest.raises(ValueError, match="lse"):
        run(mh, dtype, c, a, bias=torch.zeros(1, 1, 1, 300), lse=torch.empty(1, a, 300, device="cuda"))
    with pytest.raises(ValueError, match="broadcast"):
        run(mh, dtype, c, a, bias=torch.zeros(2, 1, 1, 300))
    with pytest.raises(ValueError, match="head_mask"):
        run(mh, dtype, c, a, hm=torch.ones(3))


# ---- module level, eval mode ---------------------------------------------------------------------------------------------------

MODE_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
LAYER_TOL = {"bf16": 2 * 2e-2, "fp32": 1e-3}


def layer_sd(rs, h, mode, prefix=""):
    """one layer's weights: the module's fp32 copy and the oracle's (linear weights as the kernels store them)"""
    sd = {}
    H.layer_weights(rs, sd, prefix, h, 4 * h, gain=1.0)
    sdt = H.to_torch(sd)
    if mode == "bf16":
        sdt = {k: (v.to(torch.bfloat16).float() if k.endswith("dense.weight") or k.split(".")[-2] in ("query", "key", "value") else v)
               for k, v in sdt.items()}
    return sdt, {k: v.double() for k, v in sdt.items()}


def load(module, sdt):
    missing, unexpected = module.load_state_dict(sdt, strict=False)
    assert not unexpected, unexpected
    return module.cuda().eval()


def oracle_layer(x, add, sd64, prefix, a, hm, gi=None):
    """O.bert_layer with the head scale between its attention and its output blocks"""
    n, s, h = x.shape
    ctx, probs = O.self_attention(x, add, sd64, prefix + "attention.self.", a, gather_index=gi)
    if hm is not None:
        probs = probs * hm.double()[None, :, None, None]
        ctx = (ctx.view(n, s, a, 64) * hm.double()[None, None, :, None]).reshape(n, s, h)
    att = O.self_output(ctx, x, sd64, prefix + "attention.output.", 1e-12)
    return O.ffn(att, sd64, prefix, 1e-12), ctx, probs


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_module_forwards_take_soft_masks_and_head_masks(mh, mode):
    """CaptionBertSelfAttention.forward (modeling_bert and the v10 class, the latter with do_chunk_cross too) and
    CaptionBertLayer.forward with a soft [N,1,S,L] mask and a head mask.  Before this route existed the mask was binarised and the
    head mask refused."""
    from modeling.modeling_bert import CaptionBertSelfAttention
    from modeling.modeling_transfomres import CaptionBertLayer
    from modeling.modeling_vcr_chunkalign_v10 import CaptionBertSelfAttention as SeqSelfAttention
    dtype = MODE_DT[mode]
    n, t, r, h, a = 3, 60, 41, 128, 2
    s = t + r
    rs = np.random.RandomState(77)
    sdt, sd64 = layer_sd(rs, h, mode)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    add = soft_bias(rs, (n, 1, s, s))
    hm = torch.tensor([0.5, 1.0])
    gi = seq_batch(np.random.RandomState(78), n, t, r)[2]
    X, A_, HM = x.to(dtype).cuda(), add.cuda(), hm.cuda()
    cfg = small_config(mode, num_hidden_layers=1)
    att_sd = {k[len("attention.self."):]: v for k, v in sdt.items() if k.startswith("attention.self.")}
    ref_y, ref_ctx, ref_p = oracle_layer(x.double(), add.double(), sd64, "", a, hm)
    with torch.no_grad():
        for cls in (CaptionBertSelfAttention, SeqSelfAttention):
            mod = load(cls(cfg), att_sd)
            ctx, probs = mod(X, A_, HM)
            check(ctx, ref_ctx, TOL[dtype], cls.__module__.split(".")[-1] + " self-attention ctx")
            check(probs, ref_p, TOL[dtype], cls.__module__.split(".")[-1] + " self-attention probs")
        _, cc_ctx, cc_p = oracle_layer(x.double(), add.double(), sd64, "", a, hm, gi=gi)
        ctx, probs = mod(X, A_, HM, do_chunk_cross=True, gather_index=[g.cuda() for g in gi])
        check(ctx, cc_ctx, TOL[dtype], "v10 self-attention ctx, do_chunk_cross")
        check(probs, cc_p, TOL[dtype], "v10 self-attention probs, do_chunk_cross")
        layer = load(CaptionBertLayer(cfg), sdt)
        y, probs = layer(X, A_, HM)
        check(y, ref_y, LAYER_TOL[mode], "layer output")
        check(probs, ref_p, TOL[dtype], "layer probs")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_binary_mask_keeps_its_route_at_module_level(mh, mode):
    """a 0 / -10000 mask with head_mask=None: forward() returns what hip_forward returns for the 0/1 key mask, bit for bit"""
    from modeling.modeling_bert import CaptionBertSelfAttention
    from modeling.modeling_transfomres import CaptionBertLayer
    dtype = MODE_DT[mode]
    n, s, h, a = 3, 101, 128, 2
    rs = np.random.RandomState(79)
    sdt, _ = layer_sd(rs, h, mode)
    X = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).cuda()
    km = torch.ones(n, s)
    km[1, 70:] = 0
    km[2] = 0
    add = O.extend_mask(km).cuda()
    cfg = small_config(mode, num_hidden_layers=1)
    layer = load(CaptionBertLayer(cfg), sdt)
    mod = layer.attention.self
    with torch.no_grad():
        c1, p1 = mod(X, add)
        c2, p2 = mod.hip_forward(X, key_mask=km.cuda(), want_probs=True)
        assert torch.equal(c1, c2) and torch.equal(p1, p2)
        y1, q1 = layer(X, add)
        y2, q2 = layer.hip_forward(X, key_mask=km.cuda(), want_probs=True)
        assert torch.equal(y1, y2) and torch.equal(q1, q2)
        # and the general route agrees with it at the bf16 bound
        c3, p3 = mod.hip_forward(X, attn_bias=add, want_probs=True)
        check(c3, c1.float(), TOL[torch.bfloat16], "general route vs binary route, ctx")
        check(p3, p1, TOL[torch.bfloat16], "general route vs binary route, probs")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_encoder_with_a_head_mask_per_layer(mh, mode):
    """CaptionBertEncoder.forward on a 3-layer config with a soft [N,1,1,L] mask and head_mask[layer] = [A], against three chained
    oracle layers"""
    from modeling.modeling_transfomres import CaptionBertEncoder
    dtype = MODE_DT[mode]
    n, s, h, a, nl = 3, 101, 128, 2, 3
    rs = np.random.RandomState(80)
    sdt, sd64 = {}, {}
    for i in range(nl):
        t_, d_ = layer_sd(rs, h, mode, "layer.%d." % i)
        sdt.update(t_)
        sd64.update(d_)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    add = soft_bias(rs, (n, 1, 1, s))
    hm = torch.tensor([[1.0, 0.5], [0.0, 1.0], [0.75, 0.25]])
    enc = load(CaptionBertEncoder(small_config(mode, num_hidden_layers=nl)), sdt)
    ref = x.double()
    for i in range(nl):
        ref = oracle_layer(ref, add.double(), sd64, "layer.%d." % i, a, hm[i])[0]
    with torch.no_grad():
        out = enc(x.to(dtype).cuda(), add.cuda(), head_mask=hm.cuda())
        out_l = enc(x.to(dtype).cuda(), add.cuda(), head_mask=[m.cuda() for m in hm])
    check(out[0], ref, LAYER_TOL[mode], "3-layer encoder, head mask tensor")
    check(out_l[0], ref, LAYER_TOL[mode], "3-layer encoder, head mask list")
