"""GPU tests of the attention forward above 256 keys (256 < P + S <= 512, eval mode: csrc/attn_long.hip behind
modcr_qkv_attn_opt_fwd): the core against the float64 oracle on the shapes a long batch produces, determinism, the refusals
(P + S > 512, dropout / row statistics / dump, a trainable layer that would need the backward), and the encoders end to end.

Bounds: max|got - ref| <= bound x max(1, max|ref|); bf16 2e-2 and fp32 1e-3 (the repository's contract), model level the
DEEP factor of tests/test_hip_models.py for 12 bf16 layers."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import modcr_oracle as O

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-3, torch.bfloat16: 2e-2}
DT = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def mh():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import modcr_hip
    modcr_hip.lib()
    return modcr_hip


def check(got, ref, tol, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    H.report_use(what, err / scale, tol)
    assert err <= tol * scale, "%s: max|err| %.4g > %.1e * %.3g" % (what, err, tol, scale)
    return err


def weights(rs, h, dtype):
    """q / k / v weights as the kernels see them (rounded to the storage dtype) and the float64 oracle's copy"""
    sd = {}
    for name in ("query", "key", "value"):
        sd[name + ".weight"] = torch.from_numpy(rs.standard_normal((h, h)).astype(np.float32) * (1.4 / np.sqrt(h)))
        sd[name + ".bias"] = torch.from_numpy(rs.standard_normal(h).astype(np.float32) * 0.1)
    for k in sd:
        if k.endswith("weight"):
            sd[k] = sd[k].to(dtype).float()
    return sd, {k: v.double() for k, v in sd.items()}


def call(mh, dtype, x, sd, a, hist=None, key_mask=None, dense=None, cid=None, align_t=0, want_probs=False):
    w = torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0).to(dtype).cuda()
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0).cuda()
    n, s, _ = x.shape
    amap = torch.zeros(n, align_t, s - align_t, device="cuda") if align_t else None
    ctx, probs = mh.qkv_attn(x.to(dtype).cuda(), w, b, key_mask=None if key_mask is None else key_mask.cuda(),
                             mask_bits=None if dense is None else mh.pack_mask_bits(dense.cuda()),
                             hist=None if hist is None else hist.to(dtype).cuda(), chunk_id=None if cid is None else cid.cuda(),
                             want_probs=want_probs, align_map=amap, align_t=align_t, num_heads=a)
    return ctx, probs, amap


def inputs(rs, n, s, p, h, dtype):
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    hist = torch.from_numpy(rs.standard_normal((n, p, h)).astype(np.float32)).to(dtype).float() if p else None
    return x, hist


# (n, s, p, h, a): the first long shapes, S = 512 exactly, the RoBERTa body (10 prefix rows + 300), Oscar-large width, an odd head count
SHAPES = [(3, 257, 0, 128, 2), (3, 300, 0, 128, 2), (2, 512, 0, 128, 2), (3, 300, 10, 128, 2), (2, 400, 0, 1024, 16),
          (3, 280, 0, 192, 3)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,s,p,h,a", SHAPES)
def test_long_attention_key_mask(mh, dtype, n, s, p, h, a):
    """broadcast key mask with ragged padded tails; sequence 1 masks every key (the reference's uniform softmax over -10000)"""
    rs = np.random.RandomState(s + 7 * p + h)
    sd, sd64 = weights(rs, h, dtype)
    x, hist = inputs(rs, n, s, p, h, dtype)
    l = p + s
    valid = rs.randint(l // 2, l + 1, size=n)
    valid[0] = l
    km = (np.arange(l)[None, :] < valid[:, None]).astype(np.float32)
    km[1] = 0
    km = torch.from_numpy(km)
    ref_ctx, ref_p = O.self_attention(x.double(), O.extend_mask(km.double()), sd64, "", a,
                                      history_state=None if hist is None else hist.double())
    ctx, probs, _ = call(mh, dtype, x, sd, a, hist=hist, key_mask=km, want_probs=(s == 300 and p == 0))
    check(ctx, ref_ctx, TOL[dtype], "ctx")
    if probs is not None:
        check(probs, ref_p, TOL[dtype], "probs")
        if dtype == torch.float32:
            assert (probs.double().sum(-1) - 1).abs().max().item() <= 1e-5
    # the production call without side outputs takes the same core
    ctx2, _, _ = call(mh, dtype, x, sd, a, hist=hist, key_mask=km)
    check(ctx2, ref_ctx, TOL[dtype], "ctx (no side outputs)")


def seq_batch(rs, n, t, r):
    """seq_enc's masks and chunk ids: text of ragged length in chunks of 1-6 tokens, ragged region counts"""
    s = t + r
    im = np.zeros((n, s), np.float32)
    cm = np.zeros((n, t, t), np.float32)
    gi = []
    for i in range(n):
        lt = int(rs.randint(t // 2, t + 1)) if i else t
        lr = int(rs.randint(r // 2, r + 1)) if i else r
        im[i, :lt] = 1
        im[i, t:t + lr] = 1
        ids, c = [], 0
        while len(ids) < lt - 2:
            ids += [c] * int(rs.randint(1, 7))
            c += 1
        ids = np.array(ids[:lt - 2])
        gi.append(torch.from_numpy(ids).to(torch.int64))
        same = ids[:, None] == ids[None, :]
        cm[i, 1:lt - 1, 1:lt - 1] = same
        cm[i, :lt, 0] = 1
        cm[i, 0, :lt] = 1
        cm[i, np.arange(lt), np.arange(lt)] = 1
    cid = torch.full((n, t), -1, dtype=torch.int32)
    for i, g in enumerate(gi):
        cid[i, 1:1 + g.numel()] = g.to(torch.int32)
    return torch.from_numpy(im), torch.from_numpy(cm), gi, cid


@pytest.mark.parametrize("dtype", DT)
def test_long_attention_seq_enc_phase_masks(mh, dtype):
    """seq_enc at T = 180, R = 100 (S = 280): the phase-1 call (dense mask) and the phase-3 call (dense mask + chunk-mean queries +
    align map), masks from modcr_build_phase_mask, against oracle.seq_phase_mask / self_attention"""
    n, t, r, h, a = 3, 180, 100, 128, 2
    rs = np.random.RandomState(180)
    sd, sd64 = weights(rs, h, dtype)
    x, _ = inputs(rs, n, t + r, 0, h, dtype)
    im, cm, gi, cid = seq_batch(rs, n, t, r)
    for phase in (1, 3):
        add = O.seq_phase_mask(im.double(), cm.double(), t, r, phase)
        bits = mh.build_phase_mask(im.cuda(), cm.cuda(), phase)
        see = torch.zeros(n, t + r, t + r, dtype=torch.bool)
        bn = bits.cpu().numpy().view(np.uint32)
        for j in range(t + r):
            see[:, :, j] = torch.from_numpy(((bn[:, :, j // 32] >> np.uint32(j % 32)) & 1).astype(bool))
        assert torch.equal(see, add[:, 0] == 0), "phase %d mask bits" % phase
        w = torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0).to(dtype).cuda()
        b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0).cuda()
        if phase == 1:
            ref_ctx, _ = O.self_attention(x.double(), add, sd64, "", a)
            ctx, _ = mh.qkv_attn(x.to(dtype).cuda(), w, b, mask_bits=bits, num_heads=a)
            check(ctx, ref_ctx, TOL[dtype], "phase-1 ctx")
        else:
            ref_ctx, ref_p = O.self_attention(x.double(), add, sd64, "", a, gather_index=gi)
            amap = torch.zeros(n, t, r, device="cuda")
            ctx, _ = mh.qkv_attn(x.to(dtype).cuda(), w, b, mask_bits=bits, chunk_id=cid.cuda(), align_map=amap, align_t=t, num_heads=a)
            check(ctx, ref_ctx, TOL[dtype], "phase-3 ctx")
            check(amap, ref_p.sum(1)[:, :t, t:], 1e-2 if dtype == torch.bfloat16 else 2e-3, "phase-3 align map")
            amap2 = torch.zeros(n, t, r, device="cuda")
            ctx2, probs = mh.qkv_attn(x.to(dtype).cuda(), w, b, mask_bits=bits, chunk_id=cid.cuda(), align_map=amap2, align_t=t,
                                      num_heads=a, want_probs=True)
            check(probs, ref_p, TOL[dtype], "phase-3 probs")
            check(amap2, ref_p.sum(1)[:, :t, t:], 1e-2 if dtype == torch.bfloat16 else 2e-3, "phase-3 align map (with probs)")


@pytest.mark.parametrize("dtype", DT)
def test_long_attention_is_deterministic(mh, dtype):
    rs = np.random.RandomState(3)
    n, s, h, a = 2, 300, 128, 2
    sd, _ = weights(rs, h, dtype)
    x, _ = inputs(rs, n, s, 0, h, dtype)
    km = torch.ones(n, s)
    km[1, 250:] = 0
    c1, p1, _ = call(mh, dtype, x, sd, a, key_mask=km, want_probs=True)
    c2, p2, _ = call(mh, dtype, x, sd, a, key_mask=km, want_probs=True)
    assert torch.equal(c1, c2) and torch.equal(p1, p2)


def test_long_attention_refusals(mh):
    """P + S = 513 names the limit; dropout, row statistics and the q|k|v dump above 256 keys are MODCR_ERR_UNSUPPORTED"""
    rs = np.random.RandomState(4)
    h, a, dtype = 128, 2, torch.bfloat16
    sd, _ = weights(rs, h, dtype)
    x, hist = inputs(rs, 1, 503, 10, h, dtype)
    with pytest.raises(ValueError, match="512"):
        call(mh, dtype, x, sd, a, hist=hist, key_mask=torch.ones(1, 513))
    n, s = 2, 300
    x = x[:, :s].to(dtype).cuda().contiguous()
    w = torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0).to(dtype).cuda()
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0).cuda()
    km = torch.ones(1, s, device="cuda")
    ctx = torch.empty_like(x)
    lib = mh.lib()
    need = lib.modcr_qkv_attn_workspace(1, s, 0, h, mh.BF16)
    assert need == 1 * s * 3 * h * 2
    assert lib.modcr_qkv_attn_workspace(1, 256, 0, h, mh.BF16) == 0            # unchanged at or below 256 keys
    ws = torch.empty(need // 4, device="cuda")
    lse = torch.empty(1, a, s, device="cuda")
    dump = torch.empty(1 * a * 3 * 192 * 64, dtype=torch.bfloat16, device="cuda")
    P = mh._ptr

    def run(attn_p=0.0, lse_=None, dump_=None):
        return lib.modcr_qkv_attn_opt_fwd(P(x), None, P(w), P(b), P(km), None, None, 0, P(ctx), None, None, 0, P(lse_), P(dump_),
                                          1, s, 0, h, a, float(attn_p), 1, 2, 0, P(ws), need, mh.BF16, mh._stream())
    assert run() == 0
    torch.cuda.synchronize()
    for kw, what in ((dict(attn_p=0.1), "dropout"), (dict(lse_=lse), "lse"), (dict(lse_=lse, dump_=dump), "dump")):
        rc = run(**kw)
        assert rc == -3, (what, rc, lib.modcr_last_error().decode())            # MODCR_ERR_UNSUPPORTED
        assert b"256" in lib.modcr_last_error()


def test_trainable_layer_above_256_keys(mh):
    """hip_autograd.BertLayerFn at S = 300: with grad enabled and parameters that want one, NotImplementedError before any launch;
    under torch.no_grad() the forward runs and matches the oracle layer"""
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    rs = np.random.RandomState(9)
    n, s, h, a = 2, 300, 128, 2
    sd = {}
    H.layer_weights(rs, sd, "", h, 4 * h)
    sdt = H.to_torch(sd)
    params = [sdt[k].clone().cuda().requires_grad_(True) for k in ag.BertLayerFn.NAMES]
    packed = hip_layers.pack_layer({k: p for k, p in zip(ag.BertLayerFn.NAMES, params)}, "", torch.device("cuda"), torch.bfloat16)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(torch.bfloat16)
    km = torch.ones(n, s)
    km[1, 220:] = 0
    xc, kmc = x.cuda(), km.cuda()
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="256"):
        ag.BertLayerFn.apply(xc, kmc, None, None, a, 1e-12, 0.0, 0.0, packed, *params)
    with torch.no_grad():
        y = ag.BertLayerFn.apply(xc, kmc, None, None, a, 1e-12, 0.0, 0.0, packed, *params)
    ref, _ = O.bert_layer(x.double(), O.extend_mask(km.double()), {k: v.to(torch.bfloat16).double() if k.endswith("weight") else v.double()
                                                                   for k, v in sdt.items()}, "", a, 1e-12)
    check(y, ref, 2 * TOL[torch.bfloat16], "trainable layer forward under no_grad")


# ---- model level, eval mode -------------------------------------------------------------------------------------------------

def small_config(mode, **kw):
    from modeling.bert_primitives import BertConfig
    d = dict(hidden_size=128, num_attention_heads=2, intermediate_size=512, num_hidden_layers=12, vocab_size=2000,
             max_position_embeddings=512, img_feature_dim=70, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
             output_attentions=True, modcr_dtype=mode, modcr_materialize_attentions=False)
    d.update(kw)
    return BertConfig(**d)


def load(module, sd_np):
    missing, unexpected = module.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    return module.cuda().eval()


MODEL_TOL = {"fp32": 1e-3, "bf16": 6e-2}        # bf16: 2e-2 x DEEP 3 of tests/test_hip_models.py (12 bf16 layers)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_encoders_above_256_keys_vs_oracle(mh, mode):
    """BertImgModel at T + R = 300 and SeqBertImgModel at T = 180, R = 100 (all three seq_enc phases, chunk-mean queries, align map),
    4 sequences, 12 layers of 64-wide heads at H = 128"""
    from Data import synthetic
    from modeling.modeling_transfomres import BertImgModel
    from modeling.modeling_vcr_chunkalign_v10 import SeqBertImgModel
    cfgd = H.cfg_dict(hidden=128, heads=2, layers=12, vocab=2000, max_pos=512, img_dim=70)
    rs = np.random.RandomState(300)
    sd_g = H.bert_img_weights(rs, cfgd, gain=1.0)
    sd_s = H.bert_img_weights(rs, cfgd, seq=True, gain=1.0)
    gm, sm = load(BertImgModel(small_config(mode)), sd_g), load(SeqBertImgModel(small_config(mode)), sd_s)
    tg, ts = H.to_torch(sd_g), H.to_torch(sd_s)
    tol = MODEL_TOL[mode]
    b = synthetic.make_batch(1, T=200, R=100, seed=31, vocab_size=2000, img_dim=70, roberta_len=8)
    assert b["input_mask"].shape[1] == 300
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    ref = O.bert_img_model(tg, "", dict(cfgd), b["input_ids"], b["token_type_ids"], b["input_mask"], b["img_feat"])
    with torch.no_grad():
        out = gm(d["input_ids"], img_feats=d["img_feat"], attention_mask=d["input_mask"], token_type_ids=d["token_type_ids"])
    check(out[0], ref[0], tol, "BertImgModel seq (300 keys)")
    check(out[1], ref[1], tol, "BertImgModel pooled (300 keys)")
    t, r = 180, 100
    b = synthetic.make_batch(1, T=t, R=r, seed=32, vocab_size=2000, img_dim=70, roberta_len=8)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    gi = [g.cuda() for g in b["gather_index"]]
    (rseq, rpool, ratt), rch = O.seq_bert_img_model(ts, "", dict(cfgd), b["input_ids"], b["token_type_ids"], b["chunk_attention_mask"],
                                                    b["input_mask"], b["img_feat"], b["gather_index"])
    rmap = torch.stack(ratt[-3:], 1).sum(1).sum(1)[:, :t, t:]
    with torch.no_grad():
        so, ch = sm(d["input_ids"], img_feats=d["img_feat"], img_mask=d["input_mask"][:, t:], input_mask=d["input_mask"],
                    attention_mask=d["chunk_attention_mask"], token_type_ids=d["token_type_ids"], offsets=None, gather_index=gi)
    check(so[0], rseq, tol, "SeqBertImgModel seq (280 keys)")
    check(so[1], rpool, tol, "SeqBertImgModel pooled")
    check(ch, rch, tol, "chunk_hidden_states")
    check(so.align_map, rmap, 4e-3 if mode == "bf16" else 2e-3, "align map (3 layers x 2 heads)")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_roberta_prefix_body_above_256_keys(mh, mode):
    """RobertaPrefixModel (Abstract_Specific's prefix body) at 260 tokens + 10 prefix vectors = 270 keys, eval under no_grad
    against oracle.roberta_prefix; with grad enabled the same call refuses (the attention backward stops at 256 keys)"""
    from modeling import hip_autograd as ag
    from modeling.roberta_prefix import RobertaPrefixModel
    torch.manual_seed(12)
    cfg = dict(vocab_size=120, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512,
               max_position_embeddings=514, type_vocab_size=2, layer_norm_eps=1e-5, pad_token_id=1)
    model = RobertaPrefixModel(**cfg, initializer_range=0.2 if mode == "fp32" else 0.05).cuda().eval()
    n, t, p = 4, 260, 10
    ids = torch.randint(3, 120, (n, t))
    ids[:, 0] = 0
    ids[1, 200:] = 1
    ids[3, 131:] = 1
    tt = torch.zeros(n, t, dtype=torch.int64)
    am = (ids != 1).float()
    prompt = torch.randn(n, p, 128) * 0.5
    pm = torch.ones(n, p)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    ref_seq, ref_pool = O.roberta_prefix(sd, "", cfg, ids, tt, am, prompt.double(), pm)
    ag.set_exact(mode == "fp32")
    try:
        with pytest.raises(NotImplementedError, match="256"):
            model(input_ids=ids.cuda(), token_type_ids=tt.cuda(), attention_mask=am.cuda(), prompt_embeddings=prompt.cuda(),
                  input_mask=pm.cuda())
        with torch.no_grad():
            seq, pool = model(input_ids=ids.cuda(), token_type_ids=tt.cuda(), attention_mask=am.cuda(), prompt_embeddings=prompt.cuda(),
                              input_mask=pm.cuda())
    finally:
        ag.set_exact(False)
    tol = 1e-3 if mode == "fp32" else 2e-2
    valid = torch.cat([am[:, :1], pm, am[:, 1:]], 1)[..., None].double()
    check(pool, ref_pool, tol, "RoBERTa body pooled (270 keys)")
    check(seq.double().cpu() * valid, ref_seq * valid, tol * (1 if mode == "fp32" else 2), "RoBERTa body sequence output (270 keys)")
