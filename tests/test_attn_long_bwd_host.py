"""CPU-side checks of the opt-in attention backward from 257 to 512 keys (modcr_qkv_attn_long_bwd, csrc/attn_long_bwd.hip): the three
symbols in both libraries, in the header and in the ctypes table; the route and workspace functions against modcr_qkv_attn_gate_bwd's
up to 256 keys and the streaming cores above; refusals of the C entry (error code and message before any launch, with never-read
pointers, so no GPU is needed) and of the Python wrapper; the hip_autograd switch (off: today's message; on: dropout, mask bits and
the align map are named); the run scripts' flag; and a float64 restatement of the STREAMED algorithm -- tile by tile, statistics,
query pass, key pass, delta = hm D -- against autograd at 1e-10."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from test_abi import header_functions

NEG_INF = float("-inf")
NARGS = {"modcr_qkv_attn_long_bwd": 33, "modcr_qkv_attn_long_bwd_workspace": 5, "modcr_qkv_attn_long_bwd_route": 6}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import modcr_hip
    return modcr_hip


def test_symbols_exported_declared_and_bound(built):
    fns = header_functions()
    for name, nargs in NARGS.items():
        assert fns.get(name) == nargs, (name, fns.get(name))
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == nargs, name
        for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    # modcr_qkv_attn_gate_bwd's argument list, in its order
    for suffix in ("", "_workspace", "_route"):
        assert built.SIGNATURES["modcr_qkv_attn_long_bwd" + suffix] == built.SIGNATURES["modcr_qkv_attn_gate_bwd" + suffix]
    assert built.ATTN_BWD_LONG_MAX_KEYS == 512 and built.ATTN_BWD_MAX_KEYS == 256


def sweep():
    """(S, P) with L = P + S from 1 to 520: no prefix, a short prefix, more prefix keys than queries"""
    for l in list(range(1, 521, 7)) + [191, 192, 193, 255, 256, 257, 258, 511, 512, 513, 520]:
        yield l, 0
        if l > 10:
            yield l - 10, 10
        if l > 64:
            yield 64, l - 64


def test_route(built):
    lib = built.lib()
    seen = set()
    for dt, stream in ((built.BF16, 3), (built.F32, 4)):
        for h, a in ((128, 2), (768, 12)):
            for s, p in sweep():
                l = s + p
                got = lib.modcr_qkv_attn_long_bwd_route(2, s, p, h, a, dt)
                if l <= 256:
                    assert got == lib.modcr_qkv_attn_gate_bwd_route(2, s, p, h, a, dt) and got in (1, 2), (s, p, dt, got)
                elif l <= 512:
                    assert got == stream, (s, p, dt, got)
                    assert lib.modcr_qkv_attn_gate_bwd_route(2, s, p, h, a, dt) == 0          # the gate entry still stops at 256
                else:
                    assert got == 0, (s, p, dt, got)
                assert built.qkv_attn_long_bwd_route(2, s, p, h, a, dt) == built.ATTN_LONG_BWD_CORES[got]
                seen.add(got)
    assert seen == {0, 1, 2, 3, 4}
    assert built.ATTN_LONG_BWD_CORES == {0: "refused", 1: "mfma", 2: "exact", 3: "stream", 4: "stream-exact"}
    for n, s, p, h, a, dt in ((2, 300, 0, 100, 2, built.BF16), (2, 300, 0, 128, 3, built.BF16), (0, 300, 0, 128, 2, built.BF16),
                              (2, 0, 300, 128, 2, built.F32), (2, 300, -1, 128, 2, built.F32), (2, 300, 0, 128, 0, built.BF16),
                              (2, 300, 0, 128, 2, 7), (2, 2 ** 31 - 1, 2, 128, 2, built.BF16)):
        assert lib.modcr_qkv_attn_long_bwd_route(n, s, p, h, a, dt) == 0, (n, s, p, h, a, dt)


def test_workspace(built):
    lib = built.lib()
    for dt in (built.BF16, built.F32):
        for h in (128, 768):
            for s, p in sweep():
                l = s + p
                need = lib.modcr_qkv_attn_long_bwd_workspace(3, s, p, h, dt)
                if l <= 256:
                    assert need == lib.modcr_qkv_attn_gate_bwd_workspace(3, s, p, h, dt) > 0, (s, p)
                elif l <= 512:
                    # the gate entry's layout (its size function does not look at the key count) + max, 1 / sum, D per query row
                    stats = 3 * (h // 64) * 3 * s * 4
                    assert need >= lib.modcr_qkv_attn_gate_bwd_workspace(3, s, p, h, dt) + stats, (s, p)
                    assert need % 256 == 0
                else:
                    assert need == 0, (s, p)
    for n, s, p, h in ((0, 300, 0, 128), (2, 0, 300, 128), (2, 300, -1, 128), (2, 300, 0, 0)):
        assert lib.modcr_qkv_attn_long_bwd_workspace(n, s, p, h, built.BF16) == 0


def long_bwd(lib, ptr, n, s, p, h, a, attn_p=0.0, bias=True, d_bias=False, d_hm=True, ws_bytes=1 << 40, dtype=0):
    """the entry with `ptr` in every pointer argument the case wants set; every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    return lib.modcr_qkv_attn_long_bwd(q, q, q if p > 0 else None, q, q, q if bias else None, 0, 0, 0, None, 0, None, 0, None, q,
                                       q if p > 0 else None, q, q, 0, q if d_bias else None, q if d_hm else None, n, s, p, h, a, attn_p, 1, 2,
                                       q, ws_bytes, dtype, None)


def test_refusals_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = [
        (dict(ptr=ptr, n=1, s=513, p=0, h=128, a=2), -3, b"512"),
        (dict(ptr=ptr, n=1, s=503, p=10, h=128, a=2), -3, b"512"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=128, a=2, attn_p=0.1), -3, b"256"),
        (dict(ptr=ptr, n=1, s=290, p=10, h=128, a=2, attn_p=0.1, dtype=1), -3, b"256"),
        (dict(ptr=0, n=1, s=300, p=0, h=128, a=2), -1, b"null pointer"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=128, a=2, bias=False, d_bias=True), -1, b"d_bias without a bias"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=100, a=2), -1, b"head size"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=128, a=2, bias=False, d_hm=False), -1, b"neither bias nor head_mask"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=128, a=2, ws_bytes=16), -1, b"workspace"),
        (dict(ptr=ptr, n=70000, s=300, p=0, h=128, a=2), -1, b"grid"),
    ]
    for kw, rc_want, text in cases:
        rc = long_bwd(lib, **kw)
        msg = lib.modcr_last_error()
        assert rc == rc_want, (kw, rc, msg)
        assert b"qkv_attn_long_bwd" in msg and text in msg, (kw, msg)
    assert b"dropout" in (long_bwd(lib, ptr=ptr, n=1, s=300, p=0, h=128, a=2, attn_p=0.1), lib.modcr_last_error())[1]
    # at 256 keys and below the call is the gate entry's: its name, its words
    assert long_bwd(lib, ptr=ptr, n=1, s=8, p=0, h=128, a=2, ws_bytes=16) == -1
    assert b"qkv_attn_gate_bwd" in lib.modcr_last_error() and b"workspace" in lib.modcr_last_error()
    # ... and the four existing entries refuse above 256 keys in the words they had
    q = ctypes.c_void_p(ptr)
    rc = lib.modcr_qkv_attn_gate_bwd(q, q, None, q, q, q, 0, 0, 0, None, 0, None, 0, None, q, None, q, q, 0, None, q, 1, 300, 0, 128, 2, 0.0, 1, 2,
                                     q, 1 << 40, 0, None)
    assert rc == -3
    assert b"qkv_attn_gate_bwd: P + S = 300 keys (P=0) exceeds the 256-key limit of the attention backward" in lib.modcr_last_error()


def test_python_wrapper_refusals_need_no_gpu(built):
    h, a = 128, 2
    w, b = torch.zeros(3 * h, h), torch.zeros(3 * h)
    nan = lambda *shape: torch.full(shape, float("nan"))
    dw, db = nan(3 * h, h), nan(3 * h)
    x513, x300 = torch.zeros(1, 513, h), torch.zeros(1, 300, h)
    hm = torch.ones(a)
    with pytest.raises(ValueError, match="512"):
        built.qkv_attn_long_bwd(x513, x513, w, b, dw, db, num_heads=a, head_mask=hm)
    with pytest.raises(ValueError, match="512"):
        built.qkv_attn_long_bwd(x300, x300, w, b, dw, db, num_heads=a, head_mask=hm, hist=torch.zeros(1, 213, h))
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn_long_bwd(x300, x300, w, b, dw, db, num_heads=a, head_mask=hm, attn_dropout=(0.1, 1, 2))
    call = lambda **kw: built.qkv_attn_long_bwd(x300, x300, w, b, dw, db, num_heads=a, **kw)
    with pytest.raises(ValueError, match="chunk_id"):
        call(head_mask=hm, hist=torch.zeros(1, 10, h), chunk_id=torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="key_mask"):
        call(attn_bias=torch.zeros(1, 1, 1, 300), key_mask=torch.ones(1, 300))
    with pytest.raises(ValueError, match="attn_bias"):
        call()
    with pytest.raises(ValueError, match="d_bias"):
        call(head_mask=hm, d_bias=torch.empty(1, a, 300, 300))
    with pytest.raises(ValueError, match="d_bias"):
        call(attn_bias=torch.zeros(1, 1, 1, 300), d_bias=torch.empty(1, a, 300, 299))
    with pytest.raises(ValueError, match="d_head_mask"):
        call(head_mask=hm, d_head_mask=nan(a))
    with pytest.raises(ValueError, match="hist"):
        call(head_mask=hm, hist=torch.zeros(2, 10, h))
    for name in ("d_align", "ctx", "lse", "dump", "mask_bits"):     # what the bias / prefix / gate route never took
        assert name not in inspect.signature(built.qkv_attn_long_bwd).parameters
    with pytest.raises(built.ModcrHipError, match="GPU"):          # a well-formed call reaches the pointer hand-over
        call(head_mask=hm)
    assert torch.isnan(dw).all() and torch.isnan(db).all()


def test_switch_off_and_on_refusals_before_any_launch():
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    assert ag.LONG_BACKWARD is False
    assert inspect.signature(hip_layers.layer_forward_train).parameters["long_backward"].default is False
    h, a = 128, 2
    x = torch.zeros(1, 300, h, requires_grad=True)
    km = torch.ones(1, 300)
    old = ("a trainable layer at S = 300 exceeds the 256 keys the attention backward takes; run it under torch.no_grad() (eval) up to "
           "512 keys")
    with pytest.raises(NotImplementedError) as e:
        ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.0, {})
    assert str(e.value) == old
    try:
        ag.set_long_backward(True)
        assert ag.LONG_BACKWARD is True
        with pytest.raises(NotImplementedError, match="256") as e:
            ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.1, {})
        assert "attention_probs_dropout_prob = 0" in str(e.value)
        with pytest.raises(NotImplementedError, match="mask_bits"):
            ag.BertLayerFn.apply(x, None, torch.zeros(1, 300, 10, dtype=torch.int32), None, a, 1e-12, 0.0, 0.0, {})
        with pytest.raises(NotImplementedError, match="align map"):
            ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.0, {"_align": (torch.zeros(1, 100, 200), 100, {})})
        with pytest.raises(NotImplementedError, match="512"):
            ag.BertLayerPrefixFn.apply(x, torch.zeros(1, 213, h), torch.zeros(1, 1, 1, 513), None, None, a, 1e-12, 0.0, 0.0, {})
        with pytest.raises(NotImplementedError, match="256"):
            ag.BertLayerGateFn.apply(x, torch.zeros(1, 10, h), None, torch.ones(a), None, a, 1e-12, 0.0, 0.1, {})
        with pytest.raises(NotImplementedError, match="256"):
            ag.BertLayerBiasFn.apply(x, torch.zeros(1, 1, 1, 300), None, None, a, 1e-12, 0.0, 0.1, {})
    finally:
        ag.set_long_backward(False)
    assert ag.LONG_BACKWARD is False
    with pytest.raises(NotImplementedError) as e:
        ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.0, {})
    assert str(e.value) == old
    # the layer function itself: the argument names the same limits
    with pytest.raises(NotImplementedError, match="attention_probs_dropout_prob = 0"):
        hip_layers.layer_forward_train({}, x.detach(), a, 1e-12, key_mask=km, attn_p=0.1, long_backward=True)
    with pytest.raises(NotImplementedError, match="mask_bits"):
        hip_layers.layer_forward_train({}, x.detach(), a, 1e-12, mask_bits=torch.zeros(1, 300, 10, dtype=torch.int32), long_backward=True)


def test_run_scripts_accept_the_flag():
    import run_PMR_ModCR as pmr
    import run_vcr_ModCR as vcr
    for mod in (pmr, vcr):
        assert mod.get_args([]).modcr_long_backward is False
        assert mod.get_args(["--modcr_long_backward"]).modcr_long_backward is True


# ---- the streamed algorithm in float64 -------------------------------------------------------------------------------------------------

def streamed_backward(q, k, v, do, bias, hm, tile=64):
    """one (sequence, head): q [S,64], k / v [L,64], do [S,64], bias [S,L] (-inf allowed), hm scalar -> (dq, dk, dv, d_bias, d_hm),
    tile by tile as csrc/attn_long_bwd.hip walks: statistics (online softmax + context accumulators -> max, 1 / sum, D without hm),
    query pass per 64-query block over the key tiles, key pass per 64-key block over the query tiles, both with delta = hm D"""
    s, l = q.shape[0], k.shape[0]
    mx, inv, dd = torch.empty(s, dtype=q.dtype), torch.empty(s, dtype=q.dtype), torch.empty(s, dtype=q.dtype)
    score = lambda i0, i1, j0, j1: q[i0:i1] @ k[j0:j1].t() / 8.0 + bias[i0:i1, j0:j1]
    for i0 in range(0, s, tile):                           # statistics pass
        i1 = min(s, i0 + tile)
        m = torch.full((i1 - i0,), NEG_INF, dtype=q.dtype)
        lsum = torch.zeros(i1 - i0, dtype=q.dtype)
        o = torch.zeros(i1 - i0, 64, dtype=q.dtype)
        for j0 in range(0, l, tile):
            j1 = min(l, j0 + tile)
            sc = score(i0, i1, j0, j1)
            mn = torch.maximum(m, sc.max(1).values)
            ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)       # every key so far at -inf: exponentials against 0
            alpha = torch.exp(m - ms)
            e = torch.exp(sc - ms[:, None])
            lsum = lsum * alpha + e.sum(1)
            o = o * alpha[:, None] + e @ v[j0:j1]
            m = mn
        mx[i0:i1] = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        inv[i0:i1] = torch.where(lsum > 0, 1.0 / lsum, torch.zeros_like(lsum))
        dd[i0:i1] = (o * do[i0:i1]).sum(1) * inv[i0:i1]   # D_i = dctx_i . (P.V)_i: no hm
    d_hm = dd.sum()
    delta = hm * dd
    dq, d_bias = torch.zeros_like(q), torch.zeros_like(bias)
    for i0 in range(0, s, tile):                           # query pass
        i1 = min(s, i0 + tile)
        for j0 in range(0, l, tile):
            j1 = min(l, j0 + tile)
            p = torch.exp(score(i0, i1, j0, j1) - mx[i0:i1, None]) * inv[i0:i1, None]
            ds = p * (hm * (do[i0:i1] @ v[j0:j1].t()) - delta[i0:i1, None])
            d_bias[i0:i1, j0:j1] = ds
            dq[i0:i1] += ds @ k[j0:j1] / 8.0
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for j0 in range(0, l, tile):                           # key pass
        j1 = min(l, j0 + tile)
        for i0 in range(0, s, tile):
            i1 = min(s, i0 + tile)
            p = torch.exp(score(i0, i1, j0, j1) - mx[i0:i1, None]) * inv[i0:i1, None]
            ds = p * (hm * (do[i0:i1] @ v[j0:j1].t()) - delta[i0:i1, None])
            dv[j0:j1] += hm * (p.t() @ do[i0:i1])
            dk[j0:j1] += ds.t() @ q[i0:i1] / 8.0
    return dq, dk, dv, d_bias, d_hm


@pytest.mark.parametrize("s,p", [(257, 0), (64, 250), (505, 7)])
def test_streamed_algorithm_in_float64(s, p):
    """against autograd of softmax(q k^T / 8 + bias) with hm as a leaf: a fully -inf query row (stood in for by a finite row with its
    dctx zeroed on the reference's side), a key hidden from every query, a head at hm = 0 whose d_hm keeps its value"""
    l, a = p + s, 2
    rs = np.random.RandomState(700 + s)
    rnd = lambda *shape: torch.from_numpy(rs.standard_normal(shape))
    q, k, v, do = rnd(a, s, 64), rnd(a, l, 64), rnd(a, l, 64), rnd(a, s, 64)
    bias = rnd(a, s, l)
    bias[rs.uniform(size=(a, s, l)) < 0.1] = -10000.0
    bias[torch.from_numpy(rs.uniform(size=(a, s, l)) < 0.1)] = NEG_INF
    bias[:, :, 0] = 0.5                                    # key 0 finite: no accidental all -inf row
    hidden = 3 if p else 70
    bias[:, :, hidden] = NEG_INF                           # a (prefix) key hidden from every query
    bias[1, 5, :] = NEG_INF                                # a query row with every key at -inf
    hm = torch.tensor([0.0, 0.75], dtype=torch.float64)   # head 0 at 0
    # reference: the all -inf row replaced by a finite one whose dctx is zero -- it then adds nothing, as the kernels' P = 0 row
    fin, dz = bias.clone(), do.clone()
    fin[1, 5, :] = 0.0
    dz[1, 5] = 0.0
    ql, kl, vl, bl, hl = (t.clone().requires_grad_(True) for t in (q, k, v, fin, hm))
    ctx = hl[:, None, None] * (torch.softmax(ql @ kl.transpose(1, 2) / 8.0 + bl, -1) @ vl)
    (ctx * dz).sum().backward()
    for h_ in range(a):
        got = streamed_backward(q[h_], k[h_], v[h_], do[h_], bias[h_], hm[h_])
        ref = [ql.grad[h_], kl.grad[h_], vl.grad[h_], bl.grad[h_].clone(), hl.grad[h_]]
        if h_ == 1:
            ref[3][5] = 0.0
        for g, r, nm in zip(got, ref, ("dq", "dk", "dv", "d_bias", "d_hm")):
            assert torch.isfinite(g).all(), (h_, nm)
            assert float((g - r).abs().max()) <= 1e-10 * max(1.0, float(r.abs().max())), (h_, nm, float((g - r).abs().max()))
        dq, dk, dv, d_bias, d_hm = got
        assert float(d_bias[:, hidden].abs().max()) == 0.0 and float(dk[hidden].abs().max()) == 0.0 and float(dv[hidden].abs().max()) == 0.0
        assert float(d_bias[torch.isinf(bias[h_])].abs().max()) == 0.0
        if h_ == 0:                                        # hm = 0: every other gradient exactly 0, d_hm formed without hm
            assert all(float(t.abs().max()) == 0.0 for t in (dq, dk, dv, d_bias))
            assert abs(float(d_hm)) > 1e-3
        else:
            assert float(d_bias[5].abs().max()) == 0.0 and float(dq[5].abs().max()) == 0.0
