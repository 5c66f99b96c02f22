"""CPU-side checks of the attention backward under an additive bias / head mask (modcr_qkv_attn_bias_bwd): the three symbols in
both libraries and in the ctypes table, the entry's argument validation (it returns its error code and a message before any
launch, so no GPU is needed), its workspace size and the route function; the Python wrappers' own refusals."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import modcr_hip
    return modcr_hip


NAMES = ("modcr_qkv_attn_bias_bwd", "modcr_qkv_attn_bias_bwd_workspace", "modcr_qkv_attn_bias_bwd_route")


def test_symbols_exported_and_in_the_table(built):
    for name in NAMES:
        assert name in built.SIGNATURES
        for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert len(built.SIGNATURES["modcr_qkv_attn_bias_bwd"][1]) == 29
    assert len(built.SIGNATURES["modcr_qkv_attn_bias_bwd_workspace"][1]) == 4
    assert len(built.SIGNATURES["modcr_qkv_attn_bias_bwd_route"][1]) == 5


def bias_bwd(lib, ptr, n, s, h, a, attn_p=0.0, bias=True, head_mask=False, d_bias=False, sn=0, sq=0, chunk_t=0, ws_bytes=1 << 40,
             ws_ptr=None, dtype=0):
    """the entry with `ptr` in every pointer argument the case wants set; every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    w = q if ws_ptr is None else ctypes.c_void_p(ws_ptr)
    return lib.modcr_qkv_attn_bias_bwd(q, q, q, q, q if bias else None, sn, 0, sq, q if head_mask else None, 0, q if chunk_t else None, chunk_t,
                                       None, q, q, q, 0, q if d_bias else None, n, s, h, a, attn_p, 1, 2, w, ws_bytes, dtype, None)


def test_argument_validation_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = [
        (dict(ptr=0, n=1, s=8, h=128, a=2), -1, b"null pointer"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, dtype=7), -1, b"dtype"),
        (dict(ptr=ptr, n=0, s=8, h=128, a=2), -1, b"bad shape"),
        (dict(ptr=ptr, n=1, s=8, h=100, a=2), -1, b"head size"),
        (dict(ptr=ptr, n=1, s=257, h=128, a=2), -3, b"256"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, bias=False), -1, b"neither bias nor head_mask"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, bias=False, head_mask=True, d_bias=True), -1, b"d_bias without a bias"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, attn_p=1.0), -1, b"[0, 1)"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, attn_p=-0.1), -1, b"[0, 1)"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, sn=-4), -1, b"negative stride"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, sq=(1 << 20) + 1), -1, b"query stride"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, chunk_t=9), -1, b"chunk_t"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, ws_bytes=16), -1, b"workspace"),
        (dict(ptr=ptr, n=1, s=8, h=128, a=2, ws_ptr=ptr + 4), -1, b"workspace"),
        (dict(ptr=ptr + 2, n=1, s=8, h=128, a=2), -1, b"align"),
    ]
    for kw, rc_want, text in cases:
        rc = bias_bwd(lib, **kw)
        msg = lib.modcr_last_error()
        assert rc == rc_want, (kw, rc, msg)
        assert b"qkv_attn_bias_bwd" in msg and text in msg, (kw, msg)


def test_workspace_is_the_binary_backward_s_and_monotone(built):
    lib = built.lib()
    for dt in (built.BF16, built.F32):
        last = 0
        for n, s in ((1, 8), (1, 37), (2, 37), (2, 180), (3, 180), (3, 256), (512, 180)):
            need = lib.modcr_qkv_attn_bias_bwd_workspace(n, s, 128, dt)
            assert need == lib.modcr_qkv_attn_bwd_workspace(n, s, 128, dt)
            assert need >= 2 * n * s * 3 * 128 * 4          # the recomputed q | k | v rows and the dq | dk | dv rows
            assert need > last
            last = need


def test_route(built):
    lib, route = built.lib(), built.qkv_attn_bias_bwd_route
    for s in (1, 37, 101, 180, 192):
        assert route(2, s, 128, 2, built.BF16) == "mfma" and lib.modcr_qkv_attn_bias_bwd_route(2, s, 128, 2, built.BF16) == 1
    for s in (193, 230, 256):
        assert route(2, s, 128, 2, built.BF16) == "exact" and lib.modcr_qkv_attn_bias_bwd_route(2, s, 128, 2, built.BF16) == 2
    for s in (1, 101, 192, 193, 256):
        assert route(2, s, 768, 12, built.F32) == "exact"
    for n, s, h, a, dt in ((2, 257, 128, 2, built.BF16), (2, 300, 128, 2, built.F32), (2, 0, 128, 2, built.BF16), (0, 8, 128, 2, built.BF16),
                           (2, 8, 100, 2, built.BF16), (2, 8, 128, 0, built.BF16), (2, 8, 128, 2, 7)):
        assert route(n, s, h, a, dt) == "refused" and lib.modcr_qkv_attn_bias_bwd_route(n, s, h, a, dt) == 0


def test_python_refusals_need_no_gpu(built):
    """the exclusivity rules of qkv_attn_bwd(attn_bias=, head_mask=, d_bias=) are checked before any tensor is touched"""
    x = torch.zeros(1, 8, 128)
    w, b, dw, db = torch.zeros(384, 128), torch.zeros(384), torch.zeros(384, 128), torch.zeros(384)
    bias = torch.zeros(1, 1, 1, 8)
    call = lambda **kw: built.qkv_attn_bwd(x, x, w, b, dw, db, num_heads=2, **kw)
    with pytest.raises(ValueError, match="key_mask"):
        call(attn_bias=bias, key_mask=torch.ones(1, 8))
    with pytest.raises(ValueError, match="key_mask"):
        call(head_mask=torch.ones(2), mask_bits=torch.zeros(1, 8, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="lse"):
        call(attn_bias=bias, ctx=x, lse=torch.zeros(1, 2, 8))
    with pytest.raises(ValueError, match="dump"):
        call(attn_bias=bias, dump=torch.zeros(4, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="d_align"):
        call(attn_bias=bias, d_align=torch.zeros(1, 3, 5), align_t=3)
    with pytest.raises(ValueError, match="broadcast"):
        call(attn_bias=torch.zeros(2, 1, 1, 8))
    with pytest.raises(ValueError, match="head_mask"):
        call(head_mask=torch.ones(3))
    with pytest.raises(ValueError, match="d_bias"):
        call(d_bias=torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError, match="d_bias"):
        call(attn_bias=bias, d_bias=torch.zeros(1, 2, 8, 7))
    x257 = torch.zeros(1, 257, 128)
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn_bwd(x257, x257, w, b, dw, db, num_heads=2, attn_bias=torch.zeros(1, 1, 1, 257))
