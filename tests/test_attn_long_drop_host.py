"""CPU-side checks of the opt-in attention-probability dropout from 257 to 512 keys (modcr_qkv_attn_long_drop_fwd / _bwd, the wide
counter layout of csrc/attn_common.h): the four symbols in both libraries, the header and the ctypes table; _route and _workspace
against modcr_qkv_attn_long_bwd's; refusals of the C entries before any launch (never-read pointers: no GPU needed); the older
entries' refusal of dropout above 256 keys, unchanged; the hip_autograd switch; the run scripts' flag; and the host restatement of
the layout (attn_wide_drop.keep): stride 512 against helpers.attn_drop_keep_torch where the two layouts share their counters, the
collision of the 256 stride that the 512 stride removes, distinct word multipliers for 64 words."""
import ctypes
import inspect

import pytest
import torch

import attn_wide_drop as W
import helpers as H
from test_abi import header_functions

NARGS = {"modcr_qkv_attn_long_drop_fwd": 29, "modcr_qkv_attn_long_drop_bwd": 33, "modcr_qkv_attn_long_drop_bwd_workspace": 5,
         "modcr_qkv_attn_long_drop_bwd_route": 6}


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
    # the argument lists of the entries they extend, in their order
    assert built.SIGNATURES["modcr_qkv_attn_long_drop_fwd"] == built.SIGNATURES["modcr_qkv_attn_bias_fwd"]
    for suffix in ("", "_workspace", "_route"):
        assert built.SIGNATURES["modcr_qkv_attn_long_drop_bwd" + suffix] == built.SIGNATURES["modcr_qkv_attn_long_bwd" + suffix]
    assert built.ATTN_DROPOUT_WIDE_MAX_KEYS == 512
    assert inspect.signature(built.qkv_attn).parameters["wide_dropout"].default is False
    assert inspect.signature(built.qkv_attn_long_bwd).parameters["wide_dropout"].default is False


def test_route_and_workspace_are_the_long_entry_s(built):
    lib = built.lib()
    seen = set()
    for dt in (built.BF16, built.F32):
        for h, a in ((128, 2), (768, 12)):
            for l in list(range(1, 521, 13)) + [192, 193, 256, 257, 511, 512, 513]:
                for s, p in ((l, 0), (l - 10, 10), (64, l - 64)):
                    if s <= 0 or p < 0:
                        continue
                    got = lib.modcr_qkv_attn_long_drop_bwd_route(2, s, p, h, a, dt)
                    assert got == lib.modcr_qkv_attn_long_bwd_route(2, s, p, h, a, dt), (s, p, dt)
                    assert lib.modcr_qkv_attn_long_drop_bwd_workspace(3, s, p, h, dt) == lib.modcr_qkv_attn_long_bwd_workspace(3, s, p, h, dt)
                    seen.add(got)
    assert seen == {0, 1, 2, 3, 4}
    assert lib.modcr_qkv_attn_long_drop_bwd_route(2, 300, 0, 100, 2, built.BF16) == 0
    assert lib.modcr_qkv_attn_long_drop_bwd_workspace(0, 300, 0, 128, built.BF16) == 0


def drop_bwd(lib, ptr, n, s, p, h, a, attn_p=0.1, ws_bytes=1 << 40, dtype=0, entry="modcr_qkv_attn_long_drop_bwd"):
    """the backward entry with `ptr` in every pointer argument; every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    return getattr(lib, entry)(q, q, q if p > 0 else None, q, q, q, 0, 0, 0, None, 0, None, 0, None, q, q if p > 0 else None, q, q, 0, None, q,
                               n, s, p, h, a, attn_p, 1, 2, q, ws_bytes, dtype, None)


def drop_fwd(lib, ptr, n, s, p, h, a, attn_p=0.1, ws_bytes=1 << 40, dtype=0, entry="modcr_qkv_attn_long_drop_fwd"):
    q = ctypes.c_void_p(ptr) if ptr else None
    return getattr(lib, entry)(q, q if p > 0 else None, q, q, q, 0, 0, 0, None, 0, None, 0, q, None, None, 0, n, s, p, h, a, attn_p, 1, 2, 0,
                               q, ws_bytes, dtype, None)


def test_refusals_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    big_a = 64                      # N * A = 65535 * 64 > 2^21 with N and A inside the grid limits
    cases = [
        (dict(ptr=ptr, n=1, s=513, p=0, h=128, a=2), -3, b"512"),
        (dict(ptr=ptr, n=1, s=503, p=10, h=128, a=2), -3, b"512"),
        (dict(ptr=ptr, n=65535, s=300, p=0, h=64 * big_a, a=big_a), -1, b"N * A = 4194240"),
        (dict(ptr=0, n=1, s=300, p=0, h=128, a=2), -1, b"null pointer"),
        (dict(ptr=ptr, n=1, s=300, p=0, h=128, a=2, ws_bytes=16), -1, b"workspace"),
    ]
    for call, who in ((drop_bwd, b"qkv_attn_long_drop_bwd"), (drop_fwd, b"qkv_attn_long_drop_fwd")):
        for kw, rc_want, text in cases:
            rc = call(lib, **kw)
            msg = lib.modcr_last_error()
            assert rc == rc_want, (kw, rc, msg)
            assert text in msg, (kw, msg)
            assert who in msg or b"512" in text, (kw, msg)
        # 2^21 itself is inside (the call then fails on its workspace, after the counter check)
        assert call(lib, ptr=ptr, n=32768, s=300, p=0, h=4096, a=64, ws_bytes=16) == -1 and b"workspace" in lib.modcr_last_error()
    # without dropout, or at 256 keys and below, the calls are the older entries': their names, their words
    assert drop_bwd(lib, ptr=ptr, n=1, s=300, p=0, h=128, a=2, attn_p=0.0, ws_bytes=16) == -1
    assert b"qkv_attn_long_bwd:" in lib.modcr_last_error() and b"workspace" in lib.modcr_last_error()
    assert drop_bwd(lib, ptr=ptr, n=1, s=8, p=0, h=128, a=2, ws_bytes=16) == -1
    assert b"qkv_attn_gate_bwd:" in lib.modcr_last_error() and b"workspace" in lib.modcr_last_error()
    for kw in (dict(s=300, attn_p=0.0), dict(s=8)):
        assert drop_fwd(lib, ptr=ptr, n=1, p=0, h=128, a=2, ws_bytes=16, **kw) == -1
        assert b"qkv_attn_bias_fwd:" in lib.modcr_last_error() and b"workspace" in lib.modcr_last_error()
    # N * A is not looked at where the wide layout does not run
    assert drop_bwd(lib, ptr=ptr, n=65535, s=8, p=0, h=4096, a=64, ws_bytes=16) == -1 and b"workspace" in lib.modcr_last_error()


def test_the_older_entries_still_refuse_dropout_at_300_keys(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    q = ctypes.c_void_p(ptr)
    assert drop_bwd(lib, ptr, 1, 300, 0, 128, 2, entry="modcr_qkv_attn_long_bwd") == -3
    assert lib.modcr_last_error() == b"qkv_attn_long_bwd: attention-probability dropout (p=0.1) is not implemented above 256 keys (P+S=300)"
    assert drop_fwd(lib, ptr, 1, 300, 0, 128, 2, entry="modcr_qkv_attn_bias_fwd") == -3
    assert lib.modcr_last_error() == b"qkv_attn_bias_fwd: attention-probability dropout (p=0.1) is not implemented above 256 keys (P+S=300)"
    # the binary-mask forward, and the older backward entries (their key limit comes first)
    rc = lib.modcr_qkv_attn_opt_fwd(q, None, q, q, q, None, None, 0, q, None, None, 0, None, None, 1, 300, 0, 128, 2, 0.1, 1, 2, 0, q, 1 << 40, 0, None)
    assert rc == -3 and b"256" in lib.modcr_last_error() and b"dropout" in lib.modcr_last_error()
    assert drop_bwd(lib, ptr, 1, 300, 0, 128, 2, entry="modcr_qkv_attn_gate_bwd") == -3 and b"256" in lib.modcr_last_error()
    # the Python wrappers, before any pointer is handed over
    h, a = 128, 2
    w, b, x = torch.zeros(3 * h, h), torch.zeros(3 * h), torch.zeros(1, 300, h)
    hm = torch.ones(a)
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn(x, w, b, num_heads=a, head_mask=hm, attn_dropout=(0.1, 1, 2))
    with pytest.raises(ValueError, match="256"):
        built.qkv_attn_long_bwd(x, x, w, b, torch.zeros(3 * h, h), torch.zeros(3 * h), num_heads=a, head_mask=hm, attn_dropout=(0.1, 1, 2))
    with pytest.raises(ValueError, match="attn_bias / head_mask"):
        built.qkv_attn(x, w, b, num_heads=a, key_mask=torch.ones(1, 300), attn_dropout=(0.1, 1, 2), wide_dropout=True)
    with pytest.raises(built.ModcrHipError, match="GPU"):           # with the opt-in a well-formed call reaches the pointer hand-over
        built.qkv_attn(x, w, b, num_heads=a, head_mask=hm, attn_dropout=(0.1, 1, 2), wide_dropout=True)
    with pytest.raises(built.ModcrHipError, match="GPU"):
        built.qkv_attn_long_bwd(x, x, w, b, torch.zeros(3 * h, h), torch.zeros(3 * h), num_heads=a, head_mask=hm, attn_dropout=(0.1, 1, 2),
                                wide_dropout=True)


def test_switch_on_with_dropout_and_back_to_off():
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    assert ag.LONG_BACKWARD is False and ag.LONG_DROPOUT is False
    assert inspect.signature(hip_layers.layer_forward_train).parameters["long_dropout"].default is False
    h, a = 128, 2
    x = torch.zeros(1, 300, h, requires_grad=True)
    km = torch.ones(1, 300)
    old = ("attention-probability dropout (p=0.1) in a trainable layer needs S <= 256 (S = 300): set attention_probs_dropout_prob = 0 to "
           "train above 256 keys")
    try:
        ag.set_long_backward(True)
        assert ag.LONG_BACKWARD is True and ag.LONG_DROPOUT is False
        with pytest.raises(NotImplementedError) as e:
            ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.1, {})
        assert str(e.value) == old
        ag.set_long_backward(True, dropout=True)
        assert ag.LONG_BACKWARD is True and ag.LONG_DROPOUT is True
        # dropout passes the switch now (the call goes on to the library, which finds no GPU tensor); what the streaming cores do not
        # carry is still named
        with pytest.raises(NotImplementedError, match="mask_bits"):
            ag.BertLayerFn.apply(x, None, torch.zeros(1, 300, 10, dtype=torch.int32), None, a, 1e-12, 0.0, 0.1, {})
        with pytest.raises(NotImplementedError, match="align map"):
            ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.1, {"_align": (torch.zeros(1, 100, 200), 100, {})})
        with pytest.raises(NotImplementedError, match="512"):
            ag.BertLayerBiasFn.apply(torch.zeros(1, 513, h, requires_grad=True), torch.zeros(1, 1, 1, 513), None, None, a, 1e-12, 0.0, 0.1, {})
        ag.set_long_backward(True)
        assert ag.LONG_DROPOUT is False
        ag.set_long_backward(True, dropout=True)
        ag.set_long_backward(False)
        assert ag.LONG_BACKWARD is False and ag.LONG_DROPOUT is False
        ag.set_long_backward(False, dropout=True)                   # dropout alone does not switch anything on
        assert ag.LONG_BACKWARD is False and ag.LONG_DROPOUT is False
    finally:
        ag.set_long_backward(False)
    with pytest.raises(NotImplementedError, match="256"):
        ag.BertLayerFn.apply(x, km, None, None, a, 1e-12, 0.0, 0.1, {})
    # hip_layers: the argument alone, and without it today's words
    with pytest.raises(NotImplementedError, match="attention_probs_dropout_prob = 0"):
        hip_layers.layer_forward_train({}, x.detach(), a, 1e-12, key_mask=km, attn_p=0.1, long_backward=True)
    with pytest.raises(NotImplementedError, match="P \\+ S <= 256"):
        hip_layers.layer_forward_train({}, x.detach(), a, 1e-12, key_mask=km, attn_p=0.1, long_dropout=True)      # (needs long_backward)
    with pytest.raises(NotImplementedError, match="mask_bits"):
        hip_layers.layer_forward_train({}, x.detach(), a, 1e-12, mask_bits=torch.zeros(1, 300, 10, dtype=torch.int32), attn_p=0.1,
                                       long_backward=True, long_dropout=True)


def test_module_route_refuses_without_the_switch():
    from modeling import hip_autograd as ag
    from modeling.modeling_bert import CaptionBertSelfAttention
    assert ag.LONG_DROPOUT is False
    src = inspect.getsource(CaptionBertSelfAttention.hip_forward)
    assert "LONG_DROPOUT" in src and "exceeds the 256 keys the attention kernels take" in src and "fold_key_mask" in src


def test_run_scripts_accept_the_flag():
    import run_PMR_ModCR as pmr
    import run_vcr_ModCR as vcr
    for mod in (pmr, vcr):
        args = mod.get_args([])
        assert args.modcr_long_dropout is False and args.modcr_long_backward is False
        args = mod.get_args(["--modcr_long_dropout"])
        assert args.modcr_long_dropout is True and args.modcr_long_backward is True          # it implies the backward switch
        args = mod.get_args(["--modcr_long_backward"])
        assert args.modcr_long_dropout is False and args.modcr_long_backward is True


# ---- the layout ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
def test_stride_512_is_the_old_layout_for_the_first_rows(p):
    """sequence 0, head 0: row = query under either stride, so below 256 queries the two layouts give the same decisions (here also
    for keys up to 512: the words beyond 31 belong to the wide layout alone, the first 32 agree)"""
    seed, off = 1234, 7 << 32
    old = H.attn_drop_keep_torch([0], 1, 250, p, seed, off, "cpu", keys=256)
    new = W.keep([0], 1, 250, p, seed, off, 512, keys=512)
    assert tuple(new.shape) == (1, 1, 250, 512)
    assert torch.equal(new[..., :256], old)
    assert torch.equal(W.keep([0], 1, 250, p, seed, off, 256, keys=256), old)
    # with more than one head the strides part: head 1's rows move
    old2 = H.attn_drop_keep_torch([0], 2, 200, p, seed, off, "cpu", keys=256)
    new2 = W.keep([0], 2, 200, p, seed, off, 512, keys=256)
    assert torch.equal(new2[:, 0], old2[:, 0]) and not torch.equal(new2[:, 1], old2[:, 1])
    frac = float(new.mean())
    assert abs(frac - (1.0 - p)) < 0.01, frac
    assert W.stride_of(256) == 256 and W.stride_of(257) == 512 and W.stride_of(512) == 512


def test_stride_512_removes_the_collision_of_stride_256():
    """(head 0, query 300) and (head 1, query 44) share their counters under stride 256 -- the layout ends at 256 queries -- and have
    distinct ones under stride 512; their keep rows differ there"""
    assert W.counters(0, 2, 0, 300, 256) == W.counters(0, 2, 1, 44, 256)
    assert not set(W.counters(0, 2, 0, 300, 512)) & set(W.counters(0, 2, 1, 44, 512))
    k256 = W.keep([0], 2, 301, 0.5, 5, 9, 256, keys=320)
    k512 = W.keep([0], 2, 301, 0.5, 5, 9, 512, keys=320)
    assert torch.equal(k256[0, 0, 300], k256[0, 1, 44])
    assert not torch.equal(k512[0, 0, 300], k512[0, 1, 44])
    # every counter of a 2-sequence, 2-head, 512-query call is distinct under stride 512
    rows = {c for n in range(2) for a in range(2) for q in range(512) for c in W.counters(n, 2, a, q, 512)}
    assert len(rows) == 2 * 2 * 512 * 4
    # the largest counter of the largest call the entries take fits 32 bits
    assert max(W.counters((1 << 21) // 2 - 1, 2, 1, 511, 512)) == 2 ** 32 - 1


def test_word_multipliers_are_distinct_for_64_words():
    cs = [H.attn_drop_const(j) for j in range(64)]
    assert len(set(cs)) == 64 and all(c & 1 for c in cs) and all(0 < c < 2 ** 32 for c in cs)
