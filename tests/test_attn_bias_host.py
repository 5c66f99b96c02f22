"""CPU-side checks of the additive-bias / head-mask attention forward (modcr_qkv_attn_bias_fwd): the binary-mask test the module
forwards use to pick a route, the two symbols in both libraries and in the ctypes table, the entry's argument validation (it
returns its error code and a message before any launch, so no GPU is needed) and its workspace size."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import modcr_hip
    return modcr_hip


def test_additive_mask_is_binary(built):
    f = built.additive_mask_is_binary
    m = torch.zeros(2, 1, 1, 9)
    assert f(m)
    m[1, 0, 0, 5:] = -10000.0
    assert f(m)
    assert f(m.double())
    soft = m.clone()
    soft[0, 0, 0, 2] = -5000.0
    assert not f(soft)
    inf = m.clone()
    inf[0, 0, 0, 2] = float("-inf")
    assert not f(inf)
    assert not f(torch.randn(2, 1, 4, 9))
    assert f(torch.zeros(0)) and isinstance(f(m), bool)


def test_symbols_exported_and_in_the_table(built):
    for name in ("modcr_qkv_attn_bias_fwd", "modcr_qkv_attn_bias_workspace"):
        assert name in built.SIGNATURES
        for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert len(built.SIGNATURES["modcr_qkv_attn_bias_fwd"][1]) == 29


def bias_fwd(lib, ptr, n, s, p, h, a, attn_p=0.0, bias=True, head_mask=False, sn=0, ws_bytes=1 << 40):
    """the entry with `ptr` in every pointer argument the case wants set; every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    return lib.modcr_qkv_attn_bias_fwd(q, q, q, q, q if bias else None, sn, 0, 0, q if head_mask else None, 0, None, 0, q, None, None, 0,
                                       n, s, p, h, a, attn_p, 1, 2, 0, q, ws_bytes, 0, None)


def test_argument_validation_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    cases = [
        (dict(ptr=0, n=1, s=8, p=0, h=128, a=2), -1, b"null pointer"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, bias=False), -1, b"neither bias nor head_mask"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=100, a=2), -1, b"head size"),
        (dict(ptr=ptr, n=1, s=503, p=10, h=128, a=2), -3, b"512"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=128, a=2, attn_p=0.1), -3, b"256"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, sn=-4), -1, b"negative stride"),
        (dict(ptr=ptr, n=1, s=8, p=0, h=128, a=2, ws_bytes=16), -1, b"workspace"),
        (dict(ptr=ptr + 2, n=1, s=8, p=0, h=128, a=2), -1, b"align"),
    ]
    for kw, rc_want, text in cases:
        rc = bias_fwd(lib, **kw)
        msg = lib.modcr_last_error()
        assert rc == rc_want, (kw, rc, msg)
        assert b"qkv_attn_bias_fwd" in msg and text in msg, (kw, msg)


def test_workspace_sizes(built):
    lib = built.lib()
    n, h = 3, 128
    for s, p in ((100, 0), (90, 10), (300, 0), (290, 10)):
        assert lib.modcr_qkv_attn_bias_workspace(n, s, p, h, built.BF16) == n * (p + s) * 3 * h * 2
        assert lib.modcr_qkv_attn_bias_workspace(n, s, p, h, built.F32) == n * (p + s) * 3 * h * 4
    # the binary routes keep theirs: nothing for the fused bf16 tile kernels, the q | k | v rows above 256 keys
    assert lib.modcr_qkv_attn_workspace(n, 256, 0, h, built.BF16) == 0
    assert lib.modcr_qkv_attn_workspace(n, 300, 0, h, built.BF16) == n * 300 * 3 * h * 2
