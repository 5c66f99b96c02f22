"""CPU-side checks of the attention backward WITH the head-mask gradient (modcr_qkv_attn_gate_bwd): the three symbols in both
libraries, in the header and in the ctypes table; the route and workspace functions against those of modcr_qkv_attn_bias_bwd (P = 0)
and modcr_qkv_attn_prefix_bwd (P > 0) over the grids tests/test_attn_prefix_bwd_host.py walks; the entry's argument validation (error
code and message before any launch, with NULL or never-read pointers, so no GPU is needed); the Python wrapper's refusals;
BertLayerGateFn's gradient slots; the older layer functions' refusal of a head mask that requires grad."""
import ctypes
import inspect

import pytest
import torch

from test_abi import header_functions


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import modcr_hip
    return modcr_hip


NARGS = {"modcr_qkv_attn_gate_bwd": 33, "modcr_qkv_attn_gate_bwd_workspace": 5, "modcr_qkv_attn_gate_bwd_route": 6}


def test_symbols_exported_declared_and_bound(built):
    fns = header_functions()
    for name, nargs in NARGS.items():
        assert fns.get(name) == nargs, (name, fns.get(name))
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == nargs, name
        for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    # modcr_qkv_attn_prefix_bwd's arguments + chunk_id, chunk_t, d_head_mask
    assert NARGS["modcr_qkv_attn_gate_bwd"] == len(built.SIGNATURES["modcr_qkv_attn_prefix_bwd"][1]) + 3


def test_route_equals_the_two_entries(built):
    lib = built.lib()
    grid = [(2, s, p, 128, 2, dt) for dt in (built.BF16, built.F32)
            for s, p in ((1, 1), (37, 5), (101, 10), (8, 120), (170, 22), (1, 191), (171, 22), (192, 1), (246, 10), (1, 255))]
    grid += [(2, s, p, 768, 12, built.F32) for s, p in ((1, 1), (101, 10), (170, 22), (171, 22), (246, 10))]
    grid += [(2, 247, 10, 128, 2, built.BF16), (2, 8, 249, 128, 2, built.F32), (2, 0, 8, 128, 2, built.BF16), (0, 8, 4, 128, 2, built.BF16),
             (2, 8, 4, 100, 2, built.BF16), (2, 8, 4, 128, 0, built.BF16), (2, 8, 4, 128, 2, 7), (2, 2 ** 31 - 1, 2, 128, 2, built.BF16)]
    seen = set()
    for n, s, p, h, a, dt in grid:
        got = lib.modcr_qkv_attn_gate_bwd_route(n, s, p, h, a, dt)
        assert got == lib.modcr_qkv_attn_prefix_bwd_route(n, s, p, h, a, dt), (n, s, p, h, a, dt)
        assert built.qkv_attn_gate_bwd_route(n, s, p, h, a, dt) == built.ATTN_BIAS_BWD_CORES[got]
        seen.add(got)
    for dt in (built.BF16, built.F32):
        for n, s, h, a in ((2, 1, 128, 2), (2, 37, 128, 2), (3, 101, 128, 2), (2, 192, 128, 2), (2, 193, 256, 4), (1, 256, 128, 2), (1, 257, 128, 2),
                           (2, 0, 128, 2), (2, 8, 100, 2)):
            got = lib.modcr_qkv_attn_gate_bwd_route(n, s, 0, h, a, dt)
            assert got == lib.modcr_qkv_attn_bias_bwd_route(n, s, h, a, dt), (n, s, h, a, dt)
            seen.add(got)
    assert seen == {0, 1, 2}
    assert lib.modcr_qkv_attn_gate_bwd_route(2, 8, -1, 128, 2, built.BF16) == 0


def test_workspace_equals_the_two_entries(built):
    lib, h = built.lib(), 128
    for dt in (built.BF16, built.F32):
        for n, s, p in ((1, 8, 1), (2, 37, 5), (2, 8, 120), (3, 101, 10), (2, 170, 22), (1, 246, 10), (512, 180, 10)):
            need = lib.modcr_qkv_attn_gate_bwd_workspace(n, s, p, h, dt)
            assert need == lib.modcr_qkv_attn_prefix_bwd_workspace(n, s, p, h, dt) > 0, (n, s, p)
            assert lib.modcr_qkv_attn_gate_bwd_workspace(n, s, 0, h, dt) == lib.modcr_qkv_attn_bias_bwd_workspace(n, s, h, dt) > 0, (n, s)
    assert lib.modcr_qkv_attn_gate_bwd_workspace(2, 8, -1, h, built.BF16) == 0
    assert lib.modcr_qkv_attn_gate_bwd_workspace(0, 8, 4, h, built.BF16) == 0


def gate_bwd(lib, ptr, n, s, p, h, a, attn_p=0.0, hist=None, d_hist=None, bias=True, head_mask=False, d_bias=False, d_hm=True, chunk=False,
             chunk_t=4, sn=0, sq=0, ws_bytes=1 << 40, ws_ptr=None, dtype=0):
    """the entry with `ptr` in every pointer argument the case wants set (hist / d_hist default to "given exactly when p > 0");
    every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    w = q if ws_ptr is None else ctypes.c_void_p(ws_ptr)
    hist = p > 0 if hist is None else hist
    d_hist = p > 0 if d_hist is None else d_hist
    return lib.modcr_qkv_attn_gate_bwd(q, q, q if hist else None, q, q, q if bias else None, sn, 0, sq, q if head_mask else None, 0,
                                       q if chunk else None, chunk_t if chunk else 0, None, q, q if d_hist else None, q, q, 0,
                                       q if d_bias else None, q if d_hm else None, n, s, p, h, a, attn_p, 1, 2, w, ws_bytes, dtype, None)


def test_argument_validation_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = [
        (dict(ptr=ptr, n=1, s=8, p=-1, h=128, a=2), -1, b"bad shape"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, hist=False), -1, b"exactly with prefix rows"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, d_hist=False), -1, b"exactly with prefix rows"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, hist=True), -1, b"exactly with prefix rows"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, d_hist=True), -1, b"exactly with prefix rows"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, chunk=True), -1, b"chunk-mean"),
        (dict(ptr=0, n=1, s=8, p=0, h=128, a=2), -1, b"null pointer"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, dtype=7), -1, b"dtype"),
        (dict(ptr=ptr, n=0, s=8, p=4, h=128, a=2), -1, b"bad shape"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=100, a=2), -1, b"head size"),
        (dict(ptr=ptr, n=1, s=257, p=0, h=128, a=2), -3, b"256"),
        (dict(ptr=ptr, n=1, s=247, p=10, h=128, a=2), -3, b"256"),
        (dict(ptr=ptr, n=1, s=8, p=249, h=128, a=2), -3, b"256"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, bias=False, d_hm=False), -1, b"neither bias nor head_mask"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, bias=False, d_bias=True), -1, b"d_bias without a bias"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, attn_p=1.0), -1, b"[0, 1)"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, sn=-4), -1, b"negative stride"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, sq=(1 << 20) + 1), -1, b"query stride"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, chunk=True, chunk_t=9), -1, b"chunk_t"),
        (dict(ptr=ptr, n=1, s=8, p=4, h=128, a=2, ws_bytes=16), -1, b"workspace"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, ws_ptr=ptr + 4), -1, b"workspace"),
        (dict(ptr=ptr + 2, n=1, s=8, p=0, h=128, a=2), -1, b"align"),
    ]
    for kw, rc_want, text in cases:
        rc = gate_bwd(lib, **kw)
        msg = lib.modcr_last_error()
        assert rc == rc_want, (kw, rc, msg)
        assert b"qkv_attn_gate_bwd" in msg and text in msg, (kw, msg)
    # head_mask == NULL and bias == NULL with d_head_mask given passes that check (the head-importance call): the next one refuses
    rc = gate_bwd(lib, ptr=ptr, n=1, s=8, p=0, h=128, a=2, bias=False, ws_bytes=16)
    assert rc == -1 and b"workspace" in lib.modcr_last_error()


def test_python_refusals_need_no_gpu(built):
    """d_head_mask is checked before any tensor is touched; without it every call goes where it went"""
    h, a, s, p = 128, 2, 8, 4
    x, hist = torch.zeros(2, s, h), torch.zeros(2, p, h)
    w, b = torch.zeros(3 * h, h), torch.zeros(3 * h)
    nan = lambda *shape: torch.full(shape, float("nan"))
    dw, db = nan(3 * h, h), nan(3 * h)
    call = lambda **kw: built.qkv_attn_bwd(x, x, w, b, dw, db, num_heads=a, **kw)
    hm = torch.ones(a)
    for bad in (nan(a), nan(2, a + 1), nan(1, a), nan(2, a, 1, 1), nan(2, a).double(), nan(a, 2).t(), nan(2, 2 * a)[:, ::2]):
        with pytest.raises(ValueError, match="d_head_mask"):
            call(head_mask=hm, d_head_mask=bad)
        with pytest.raises(ValueError, match="d_head_mask"):
            call(head_mask=hm, hist=hist, d_head_mask=bad)
        assert torch.isnan(bad).all()
    d_hm = nan(2, a)
    with pytest.raises(ValueError, match="key_mask"):
        call(d_head_mask=d_hm, key_mask=torch.ones(2, s))
    with pytest.raises(ValueError, match="lse"):
        call(d_head_mask=d_hm, ctx=x, lse=torch.zeros(2, a, s))
    with pytest.raises(ValueError, match="chunk_id"):
        call(head_mask=hm, hist=hist, d_head_mask=d_hm, chunk_id=torch.zeros(2, 4, dtype=torch.int32))
    x257 = torch.zeros(1, 257, h)
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn_bwd(x257, x257, w, b, dw, db, num_heads=a, head_mask=hm, d_head_mask=nan(1, a))
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn_bwd(x257[:, :247], x257[:, :247], w, b, dw, db, num_heads=a, head_mask=hm, hist=torch.zeros(1, 10, h), d_head_mask=nan(1, a))
    with pytest.raises(built.ModcrHipError, match="GPU"):          # a well-formed call reaches the pointer hand-over
        call(head_mask=hm, d_head_mask=d_hm)
    assert torch.isnan(dw).all() and torch.isnan(db).all() and torch.isnan(d_hm).all()


def test_layer_backward_takes_want_d_head_mask(built):
    from modeling import hip_layers
    assert "want_d_head_mask" in inspect.signature(hip_layers.layer_backward).parameters
    assert inspect.signature(hip_layers.layer_backward).parameters["want_d_head_mask"].default is False


def test_gate_fn_returns_one_gradient_slot_per_input():
    """BertLayerGateFn.backward: dx, d_hist, d_bias, d_head_mask, six Nones and the 16 parameter gradients, in the order of forward's
    inputs (BertLayerPrefixFn's); the [N, A] head-mask gradient is summed to the mask's own shape and cast to its dtype"""
    from modeling import hip_autograd as ag
    names = list(inspect.signature(ag.BertLayerGateFn.forward).parameters)
    assert names == list(inspect.signature(ag.BertLayerPrefixFn.forward).parameters)
    n, a, s, p, h = 3, 2, 8, 4, 128

    class Ctx(object):
        pass
    d_hm = torch.arange(n * a, dtype=torch.float32).reshape(n, a) + 1.0
    grads = tuple(torch.zeros(1) for _ in ag.BertLayerFn.NAMES)
    orig = ag._bert_layer_backward
    try:
        for shape, dtype in (((a,), torch.float32), ((n, a), torch.float32), ((1, a, 1, 1), torch.float64), ((n, a, 1, 1), torch.bfloat16),
                             ((1, a), torch.float32)):
            ctx = Ctx()
            ctx.bias_shape, ctx.need_hist, ctx.hm_shape = ((n, 1, 1, p + s), torch.float32), False, (shape, dtype)

            def fake_backward(c, dy):
                c.d_hist, c.d_hm = torch.zeros(n, p, h), d_hm
                return dy, grads, torch.ones(n, a, s, p + s)
            ag._bert_layer_backward = fake_backward
            out = ag.BertLayerGateFn.backward(ctx, torch.zeros(n, s, h))
            assert len(out) == 10 + len(ag.BertLayerFn.NAMES)
            assert out[1] is None and ctx.d_hist is None and ctx.d_hm is None
            assert tuple(out[2].shape) == (n, 1, 1, p + s)
            assert tuple(out[3].shape) == shape and out[3].dtype == dtype
            want = d_hm if shape[0] == n and len(shape) > 1 else d_hm.sum(0)
            assert torch.equal(out[3].float().reshape(want.shape), want.to(dtype).float())
            assert all(o is None for o in out[4:10]) and out[10:] == grads
    finally:
        ag._bert_layer_backward = orig


def test_older_layer_functions_still_refuse_a_head_mask_that_requires_grad():
    """the shared forward's check is lifted by a flag that BertLayerGateFn alone sets; the check sits before any launch"""
    from modeling import hip_autograd as ag
    h, a = 128, 2
    x = torch.zeros(1, 8, h, requires_grad=True)
    hm = torch.ones(a, requires_grad=True)
    with pytest.raises(NotImplementedError, match="head_mask"):
        ag.BertLayerBiasFn.apply(x, None, hm, None, a, 1e-12, 0.0, 0.0, {})
    with pytest.raises(NotImplementedError, match="head_mask"):
        ag.BertLayerPrefixFn.apply(x, torch.zeros(1, 4, h), None, hm, None, a, 1e-12, 0.0, 0.0, {})
    with pytest.raises(ValueError, match="head_mask"):
        ag.BertLayerGateFn.apply(x, None, torch.zeros(1, 1, 1, 8), None, None, a, 1e-12, 0.0, 0.0, {})
    with pytest.raises(ValueError, match="chunk-mean"):
        ag.BertLayerGateFn.apply(x, torch.zeros(1, 4, h), None, hm, torch.zeros(1, 4, dtype=torch.int32), a, 1e-12, 0.0, 0.0, {})
    src = inspect.signature(ag._bert_layer_forward).parameters
    assert src["head_mask_grad"].default is False
