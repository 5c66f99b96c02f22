"""CPU-side checks of the attention backward with prefix rows (modcr_qkv_attn_prefix_bwd, history states): the three symbols in
both libraries, in the header and in the ctypes table with matching argument counts; the entry's argument validation (error code
and message before any launch, so no GPU is needed), its workspace size and the route function; _bias_strides with the key
dimension L = P + S; the host fold of a binary key mask; the Python wrappers' own refusals; BertLayerPrefixFn's gradient slots."""
import ctypes

import pytest
import torch

from test_abi import header_functions


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import modcr_hip
    return modcr_hip


NARGS = {"modcr_qkv_attn_prefix_bwd": 30, "modcr_qkv_attn_prefix_bwd_workspace": 5, "modcr_qkv_attn_prefix_bwd_route": 6}


def test_symbols_exported_declared_and_bound(built):
    fns = header_functions()
    for name, nargs in NARGS.items():
        assert fns.get(name) == nargs, (name, fns.get(name))
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == nargs, name
        for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)


def prefix_bwd(lib, ptr, n, s, p, h, a, attn_p=0.0, hist=True, bias=True, head_mask=False, d_bias=False, sn=0, sq=0, ws_bytes=1 << 40,
               ws_ptr=None, dtype=0):
    """the entry with `ptr` in every pointer argument the case wants set; every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    w = q if ws_ptr is None else ctypes.c_void_p(ws_ptr)
    return lib.modcr_qkv_attn_prefix_bwd(q, q, q if hist else None, q, q, q if bias else None, sn, 0, sq, q if head_mask else None, 0, None,
                                         q, q, q, q, 0, q if d_bias else None, n, s, p, h, a, attn_p, 1, 2, w, ws_bytes, dtype, None)


def test_argument_validation_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = [
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2), -1, b"modcr_qkv_attn_bias_bwd"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, hist=False), -1, b"modcr_qkv_attn_bias_bwd"),
        (dict(ptr=0, n=1, s=8, p=4, h=128, a=2), -1, b"modcr_qkv_attn_bias_bwd"),          # (hist is null too)
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, dtype=7), -1, b"dtype"),
        (dict(ptr=ptr, n=0, s=8, p=4, h=128, a=2), -1, b"bad shape"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=100, a=2), -1, b"head size"),
        (dict(ptr=ptr, n=1, s=247, p=10, h=128, a=2), -3, b"256"),
        (dict(ptr=ptr, n=1, s=8, p=249, h=128, a=2), -3, b"256"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, bias=False), -1, b"neither bias nor head_mask"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, bias=False, head_mask=True, d_bias=True), -1, b"d_bias without a bias"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, attn_p=1.0), -1, b"[0, 1)"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, sn=-4), -1, b"negative stride"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, sq=(1 << 20) + 1), -1, b"query stride"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, ws_bytes=16), -1, b"workspace"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, ws_ptr=ptr + 4), -1, b"workspace"),
        (dict(ptr=ptr + 2, n=1, s=8, p=4, h=128, a=2), -1, b"align"),
    ]
    for kw, rc_want, text in cases:
        rc = prefix_bwd(lib, **kw)
        msg = lib.modcr_last_error()
        assert rc == rc_want, (kw, rc, msg)
        assert b"qkv_attn_prefix_bwd" in msg and text in msg, (kw, msg)


def test_workspace_holds_both_row_sets_and_both_gemm_sets(built):
    lib = built.lib()
    h = 128
    for dt in (built.BF16, built.F32):
        for n, s, p in ((1, 8, 1), (2, 37, 5), (2, 8, 120), (3, 101, 10), (2, 170, 22), (1, 246, 10), (512, 180, 10)):
            need = lib.modcr_qkv_attn_prefix_bwd_workspace(n, s, p, h, dt)
            rows = 2 * n * s * 3 * h * 4 + 2 * n * p * 2 * h * 4
            sub = max(lib.modcr_linear_bwd_input_workspace(n * s, 3 * h, h), lib.modcr_linear_bwd_weight_workspace(n * s, 3 * h, h),
                      lib.modcr_linear_bwd_input_workspace(n * p, 2 * h, h), lib.modcr_linear_bwd_weight_workspace(n * p, 2 * h, h))
            assert need >= rows + sub, (n, s, p, need, rows, sub)
            assert need > lib.modcr_qkv_attn_bias_bwd_workspace(n, s, h, dt)
    assert lib.modcr_qkv_attn_prefix_bwd_workspace(2, 8, 0, h, built.BF16) == 0


def test_route(built):
    lib, route = built.lib(), built.qkv_attn_prefix_bwd_route
    for s, p in ((1, 1), (37, 5), (101, 10), (8, 120), (170, 22), (1, 191)):
        assert route(2, s, p, 128, 2, built.BF16) == "mfma" and lib.modcr_qkv_attn_prefix_bwd_route(2, s, p, 128, 2, built.BF16) == 1
    for s, p in ((171, 22), (192, 1), (246, 10), (1, 255)):
        assert route(2, s, p, 128, 2, built.BF16) == "exact" and lib.modcr_qkv_attn_prefix_bwd_route(2, s, p, 128, 2, built.BF16) == 2
    for s, p in ((1, 1), (101, 10), (170, 22), (171, 22), (246, 10)):
        assert route(2, s, p, 768, 12, built.F32) == "exact"
    for n, s, p, h, a, dt in ((2, 247, 10, 128, 2, built.BF16), (2, 8, 249, 128, 2, built.F32), (2, 8, 0, 128, 2, built.BF16),
                              (2, 0, 8, 128, 2, built.BF16), (0, 8, 4, 128, 2, built.BF16), (2, 8, 4, 100, 2, built.BF16),
                              (2, 8, 4, 128, 0, built.BF16), (2, 8, 4, 128, 2, 7), (2, 2 ** 31 - 1, 2, 128, 2, built.BF16)):
        assert route(n, s, p, h, a, dt) == "refused" and lib.modcr_qkv_attn_prefix_bwd_route(n, s, p, h, a, dt) == 0


def test_bias_strides_with_key_dimension_l(built):
    n, a, s, p = 2, 2, 8, 5
    l = p + s
    f = built._bias_strides
    b, st = f(torch.zeros(n, a, s, l), n, a, s, l)
    assert st == [a * s * l, s * l, l] and b.stride(3) == 1
    b, st = f(torch.zeros(n, 1, 1, l), n, a, s, l)
    assert st == [l, 0, 0]
    b, st = f(torch.zeros(1, a, s, l), n, a, s, l)
    assert st == [0, s * l, l]
    view = torch.zeros(n, 1, 1, l).expand(n, a, s, l)                   # an expand()ed view stays a view
    b, st = f(view, n, a, s, l)
    assert b.data_ptr() == view.data_ptr() and st == [l, 0, 0]
    wide = torch.zeros(n, a, s, l + 3)[..., :l]                         # rows of a wider tensor: the row stride is kept
    b, st = f(wide, n, a, s, l)
    assert b.data_ptr() == wide.data_ptr() and st == [a * s * (l + 3), s * (l + 3), l + 3]
    with pytest.raises(ValueError, match="P \\+ S = 13"):
        f(torch.zeros(n, 1, 1, s), n, a, s, l)                          # the key dimension must be L, not S


def test_mask_fold(built):
    km = torch.tensor([[1.0, 1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 1.0, 1.0]])
    add = built.fold_key_mask(km)
    assert tuple(add.shape) == (2, 1, 1, 5) and add.dtype == torch.float32
    assert torch.equal(add.reshape(2, 5), torch.where(km > 0, torch.zeros(()), torch.full((), -10000.0)))
    assert built.additive_mask_is_binary(add)
    assert torch.equal(built.fold_key_mask(km.to(torch.int64)), add)
    with pytest.raises(ValueError, match="key_mask"):
        built.fold_key_mask(torch.ones(2, 1, 1, 5))


def test_python_refusals_need_no_gpu(built):
    """the exclusivity rules and limits of qkv_attn_bwd(hist=) are checked before any tensor is touched"""
    h, a, s, p = 128, 2, 8, 4
    x, hist = torch.zeros(1, s, h), torch.zeros(1, p, h)
    w, b = torch.zeros(3 * h, h), torch.zeros(3 * h)
    nan = lambda *shape: torch.full(shape, float("nan"))
    dw, db = nan(3 * h, h), nan(3 * h)
    bias = torch.zeros(1, 1, 1, p + s)
    call = lambda **kw: built.qkv_attn_bwd(x, x, w, b, dw, db, num_heads=a, hist=hist, **kw)
    with pytest.raises(ValueError, match="lse"):
        call(attn_bias=bias, ctx=x, lse=torch.zeros(1, a, s))
    with pytest.raises(ValueError, match="dump"):
        call(attn_bias=bias, dump=torch.zeros(4, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="d_align"):
        call(attn_bias=bias, d_align=torch.zeros(1, 3, 5), align_t=3)
    with pytest.raises(ValueError, match="chunk_id"):
        call(attn_bias=bias, chunk_id=torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_bits"):
        call(mask_bits=torch.zeros(1, s, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="key_mask"):
        call(attn_bias=bias, key_mask=torch.ones(1, p + s))
    with pytest.raises(ValueError, match="P \\+ S = 12"):
        call(attn_bias=torch.zeros(1, 1, 1, s))                         # a bias over the own keys only
    with pytest.raises(ValueError, match="P \\+ S = 12"):
        call(key_mask=torch.ones(1, s))                                 # ... and a key mask over them
    with pytest.raises(ValueError, match="d_bias"):
        call(attn_bias=bias, d_bias=torch.zeros(1, a, s, s))            # [N, A, S, S]: the shape without prefix rows
    with pytest.raises(ValueError, match="d_bias"):
        call(head_mask=torch.ones(a), d_bias=torch.zeros(1, a, s, p + s))
    with pytest.raises(ValueError, match="head_mask"):
        call()
    with pytest.raises(ValueError, match="hist"):
        built.qkv_attn_bwd(x, x, w, b, dw, db, num_heads=a, hist=torch.zeros(2, p, h), attn_bias=bias)
    with pytest.raises(ValueError, match="hist"):
        built.qkv_attn_bwd(x, x, w, b, dw, db, num_heads=a, hist=torch.zeros(1, p, h, dtype=torch.bfloat16), attn_bias=bias)
    x247 = torch.zeros(1, 247, h)
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn_bwd(x247, x247, w, b, dw, db, num_heads=a, hist=torch.zeros(1, 10, h), attn_bias=torch.zeros(1, 1, 1, 257))
    assert torch.isnan(dw).all() and torch.isnan(db).all()


def test_layer_forward_train_refusals_need_no_gpu(built):
    from modeling import hip_layers
    h, a = 128, 2
    x, hist = torch.zeros(1, 8, h), torch.zeros(1, 4, h)
    with pytest.raises(ValueError, match="hist"):
        hip_layers.layer_forward_train({}, x, a, 1e-12, hist=hist)
    with pytest.raises(ValueError, match="mask_bits"):
        hip_layers.layer_forward_train({}, x, a, 1e-12, hist=hist, mask_bits=torch.zeros(1, 8, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="key_mask"):
        hip_layers.layer_forward_train({}, x, a, 1e-12, hist=hist, key_mask=torch.ones(1, 12), attn_bias=torch.zeros(1, 1, 1, 12))


def test_prefix_fn_returns_one_gradient_slot_per_input():
    """BertLayerPrefixFn.backward: dx, d_hist, d_bias, seven Nones and the 16 parameter gradients, in the order of forward's inputs;
    the bias gradient is summed to the bias's own shape"""
    import inspect
    from modeling import hip_autograd as ag
    names = list(inspect.signature(ag.BertLayerPrefixFn.forward).parameters)
    assert names[:11] == ["ctx", "x", "hist", "attn_bias", "head_mask", "chunk_id", "num_heads", "eps", "p", "attn_p", "packed"]
    n, a, s, p, h = 2, 2, 8, 4, 128

    class Ctx(object):
        pass
    ctx = Ctx()
    ctx.bias_shape, ctx.need_hist = ((n, 1, 1, p + s), torch.float32), True
    dense = torch.ones(n, a, s, p + s)
    d_hist = torch.zeros(n, p, h)
    grads = tuple(torch.zeros(1) for _ in ag.BertLayerFn.NAMES)

    def fake_backward(c, dy):
        c.d_hist = d_hist
        return dy, grads, dense
    orig = ag._bert_layer_backward
    ag._bert_layer_backward = fake_backward
    try:
        out = ag.BertLayerPrefixFn.backward(ctx, torch.zeros(n, s, h))
        ctx.need_hist = False
        out2 = ag.BertLayerPrefixFn.backward(ctx, torch.zeros(n, s, h))
    finally:
        ag._bert_layer_backward = orig
    assert len(out) == 10 + len(ag.BertLayerFn.NAMES)
    assert out[1] is d_hist and out2[1] is None and ctx.d_hist is None
    assert tuple(out[2].shape) == (n, 1, 1, p + s) and float(out[2][0, 0, 0, 0]) == a * s
    assert all(o is None for o in out[3:10]) and out[10:] == grads
