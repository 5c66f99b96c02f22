"""CPU-side checks of the opt-in dense mask bits and align-map gradient from 257 to 512 keys (modcr_qkv_attn_long_align_fwd / _bwd):
the symbols in both libraries, the header and the ctypes table; _route and _workspace against modcr_qkv_attn_long_drop_bwd's over a
grid of shapes; every refusal of the C entries by code and message (never-read pointers: no GPU needed); qkv_attn(mask_bits=,
attn_bias=) still raising; the hip_autograd switch; the two NotImplementedError texts with `align` off; and a float64 restatement of
the query kernel's sweep-1 accumulator (running max, rescale, final divide) against the direct sum."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from test_abi import header_functions

NARGS = {"modcr_qkv_attn_long_align_fwd": 30, "modcr_qkv_attn_long_align_bwd": 37, "modcr_qkv_attn_long_align_bwd_workspace": 5,
         "modcr_qkv_attn_long_align_bwd_route": 6}


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
    # the drop entries' argument lists in their order, then the new arguments
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert built.SIGNATURES["modcr_qkv_attn_long_align_fwd"][1] == built.SIGNATURES["modcr_qkv_attn_long_drop_fwd"][1] + [vp]
    assert built.SIGNATURES["modcr_qkv_attn_long_align_bwd"][1] == built.SIGNATURES["modcr_qkv_attn_long_drop_bwd"][1] + [vp, vp, i32, i32]
    for suffix in ("_workspace", "_route"):
        assert built.SIGNATURES["modcr_qkv_attn_long_align_bwd" + suffix] == built.SIGNATURES["modcr_qkv_attn_long_drop_bwd" + suffix]
    assert built.ATTN_LONG_ALIGN_MAX_KEYS == 512
    assert inspect.signature(built.qkv_attn).parameters["dense_bits"].default is None


def test_route_and_workspace_are_the_drop_entry_s(built):
    lib = built.lib()
    seen = set()
    for dt in (built.BF16, built.F32):
        for h, a in ((128, 2), (768, 12)):
            for l in list(range(1, 521, 13)) + [192, 193, 256, 257, 511, 512, 513]:
                for s, p in ((l, 0), (l - 10, 10), (64, l - 64)):
                    if s <= 0 or p < 0:
                        continue
                    got = lib.modcr_qkv_attn_long_align_bwd_route(2, s, p, h, a, dt)
                    assert got == lib.modcr_qkv_attn_long_drop_bwd_route(2, s, p, h, a, dt), (s, p, dt)
                    assert lib.modcr_qkv_attn_long_align_bwd_workspace(3, s, p, h, dt) == lib.modcr_qkv_attn_long_drop_bwd_workspace(3, s, p, h, dt)
                    seen.add(got)
                    if got:
                        assert built.qkv_attn_long_align_bwd_route(2, s, p, h, a, dt) == built.ATTN_LONG_BWD_CORES[got]
    assert seen == {0, 1, 2, 3, 4}
    assert lib.modcr_qkv_attn_long_align_bwd_route(2, 300, 0, 100, 2, built.BF16) == 0
    assert lib.modcr_qkv_attn_long_align_bwd_workspace(0, 300, 0, 128, built.BF16) == 0


def align_bwd(lib, ptr, n, s, p, h, a, bits=None, d_align=None, align_t=0, flags=0, attn_p=0.1, ws_bytes=1 << 40, dtype=0, bias=True):
    """the backward entry with `ptr` in every pointer argument; every case here fails validation, so nothing is read"""
    q = ctypes.c_void_p(ptr) if ptr else None
    vp = lambda v: ctypes.c_void_p(v) if v else None
    return lib.modcr_qkv_attn_long_align_bwd(q, q, q if p > 0 else None, q, q, q if bias else None, 0, 0, 0, None, 0, None, 0, None, q,
                                             q if p > 0 else None, q, q, 0, None, None, n, s, p, h, a, attn_p, 1, 2, q, ws_bytes, dtype, None,
                                             vp(bits), vp(d_align), align_t, flags)


def align_fwd(lib, ptr, n, s, p, h, a, bits=None, attn_p=0.1, ws_bytes=1 << 40, dtype=0, bias=True):
    q = ctypes.c_void_p(ptr) if ptr else None
    return lib.modcr_qkv_attn_long_align_fwd(q, q if p > 0 else None, q, q, q if bias else None, 0, 0, 0, None, 0, None, 0, q, None, None, 0,
                                             n, s, p, h, a, attn_p, 1, 2, 0, q, ws_bytes, dtype, None, ctypes.c_void_p(bits) if bits else None)


def test_refusals_before_any_launch(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    err = lib.modcr_last_error
    shape = dict(ptr=ptr, n=1, h=128, a=2)
    who = b"qkv_attn_long_align_bwd: "
    # bits or d_align with prefix rows
    for kw in (dict(bits=ptr), dict(d_align=ptr, align_t=10)):
        assert align_bwd(lib, s=300, p=10, **shape, **kw) == -1 and err().startswith(who) and b"prefix rows (P=10" in err()
    assert align_fwd(lib, s=300, p=10, bits=ptr, **shape) == -1 and b"qkv_attn_long_align_fwd: no mask_bits with prefix rows (P=10" in err()
    # ... at 256 keys and below: unsupported, naming 256 and the entry that serves them there
    for s in (8, 256):
        for kw in (dict(bits=ptr), dict(d_align=ptr, align_t=4)):
            assert align_bwd(lib, s=s, p=0, **shape, **kw) == -3
            assert err().startswith(who) and b"256" in err() and b"modcr_qkv_attn_bwd" in err() and b"lse" in err()
        assert align_fwd(lib, s=s, p=0, bits=ptr, **shape) == -3 and b"256" in err() and b"modcr_qkv_attn_opt_fwd" in err()
    # d_align without 0 < align_t < S
    for t in (0, -1, 300, 301):
        assert align_bwd(lib, s=300, p=0, d_align=ptr, align_t=t, **shape) == -1
        assert err() == who + b"align_t=%d out of range" % t
    # pointers off 4 bytes, unknown flags
    assert align_bwd(lib, s=300, p=0, bits=ptr + 2, **shape) == -1 and err() == who + b"mask_bits / d_align not 4-byte aligned"
    assert align_bwd(lib, s=300, p=0, d_align=ptr + 1, align_t=100, **shape) == -1 and b"4-byte aligned" in err()
    assert align_fwd(lib, s=300, p=0, bits=ptr + 2, **shape) == -1 and err() == b"qkv_attn_long_align_fwd: mask_bits not 4-byte aligned"
    assert align_bwd(lib, s=300, p=0, bits=ptr, flags=2, **shape) == -1 and err() == who + b"unknown flags 0x2"
    # what the drop entry refuses: its checks, under the new entry's name where the bits or d_align make it the new entry's call
    cases = [(dict(s=513), -3, b"512"), (dict(s=300, ws_bytes=16), -1, b"workspace"), (dict(s=300, dtype=7), -1, b"unknown dtype")]
    for kw, rc, text in cases:
        assert align_bwd(lib, p=0, bits=ptr, **shape, **kw) == rc and text in err() and err().startswith(who), err()
        assert align_fwd(lib, p=0, bits=ptr, **shape, **kw) == rc and text in err(), err()
    assert align_bwd(lib, ptr=ptr, n=65535, s=300, p=0, h=4096, a=64, bits=ptr) == -1 and b"N * A = 4194240" in err()
    assert align_bwd(lib, ptr=0, n=1, s=300, p=0, h=128, a=2, bits=ptr) == -1 and b"null pointer" in err()
    # "neither bias nor head_mask" is satisfied by the bits, not by d_align alone
    assert align_bwd(lib, s=300, p=0, bits=ptr, bias=False, ws_bytes=16, **shape) == -1 and b"workspace" in err()
    assert align_fwd(lib, s=300, p=0, bits=ptr, bias=False, ws_bytes=16, **shape) == -1 and b"workspace" in err()
    assert align_bwd(lib, s=300, p=0, d_align=ptr, align_t=100, bias=False, **shape) == -1 and b"neither bias nor head_mask" in err()
    # with neither it IS the drop entry's call: its names, its words, at every key count
    import test_attn_long_drop_host as D
    for kw in (dict(s=300, ws_bytes=16), dict(s=300, attn_p=0.0, ws_bytes=16), dict(s=8, ws_bytes=16), dict(s=513), dict(s=300, dtype=7)):
        rc = align_bwd(lib, p=0, **shape, **kw)
        msg = err()
        assert (rc, msg) == (D.drop_bwd(lib, p=0, **shape, **kw), err())
        assert b"long_align" not in msg
        rc = align_fwd(lib, p=0, **shape, **kw)
        msg = err()
        assert (rc, msg) == (D.drop_fwd(lib, p=0, **shape, **kw), err())
        assert b"long_align" not in msg


def test_python_wrappers_before_any_pointer_is_handed_over(built):
    h, a = 128, 2
    w, b, x = torch.zeros(3 * h, h), torch.zeros(3 * h), torch.zeros(1, 300, h)
    bits = torch.zeros(1, 300, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="attn_bias / head_mask replace key_mask / mask_bits"):
        built.qkv_attn(x, w, b, num_heads=a, mask_bits=bits, attn_bias=torch.zeros(1, 1, 1, 300))
    with pytest.raises(ValueError, match="dense_bits must be a contiguous int32"):
        built.qkv_attn(x, w, b, num_heads=a, dense_bits=bits[:, :, :9])
    with pytest.raises(built.ModcrHipError, match="GPU"):           # dense_bits alone selects the route: a well-formed call reaches the hand-over
        built.qkv_attn(x, w, b, num_heads=a, dense_bits=bits)
    dw, db = torch.zeros(3 * h, h), torch.zeros(3 * h)
    with pytest.raises(ValueError, match="d_align must be a contiguous fp32"):
        built.qkv_attn_long_bwd(x, x, w, b, dw, db, num_heads=a, dense_bits=bits, d_align=torch.zeros(1, 100, 199), align_t=100)
    with pytest.raises(TypeError, match="unexpected keyword"):
        built.qkv_attn_long_bwd(x, x, w, b, dw, db, num_heads=a, mask_bits=bits)
    with pytest.raises(built.ModcrHipError, match="GPU"):
        built.qkv_attn_long_bwd(x, x, w, b, dw, db, num_heads=a, dense_bits=bits, d_align=torch.zeros(1, 100, 200), align_t=100)


def test_switch_and_refusal_texts():
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    assert ag.LONG_ALIGN is False
    assert inspect.signature(ag.set_long_backward).parameters["align"].default is False
    assert inspect.signature(hip_layers.layer_forward_train).parameters["long_align"].default is False
    try:
        ag.set_long_backward(True)
        assert (ag.LONG_BACKWARD, ag.LONG_DROPOUT, ag.LONG_ALIGN) == (True, False, False)
        ag.set_long_backward(True, dropout=True)
        assert (ag.LONG_BACKWARD, ag.LONG_DROPOUT, ag.LONG_ALIGN) == (True, True, False)
        ag.set_long_backward(True, align=True)
        assert (ag.LONG_BACKWARD, ag.LONG_DROPOUT, ag.LONG_ALIGN) == (True, False, True)
        ag.set_long_backward(False, dropout=True, align=True)
        assert (ag.LONG_BACKWARD, ag.LONG_DROPOUT, ag.LONG_ALIGN) == (False, False, False)
        # align off: the two refusals, word for word
        ag.set_long_backward(True, dropout=True)
        h, a = 128, 2
        x = torch.zeros(1, 300, h, requires_grad=True)
        bits = torch.zeros(1, 300, 10, dtype=torch.int32)
        names = list(ag.BertLayerFn.NAMES)
        packed = {}
        with pytest.raises(NotImplementedError) as e:
            ag._bert_layer_forward(None, x, None, a, 1e-12, 0.0, 0.0, packed, [], mask_bits=bits)
        assert str(e.value) == ("the streaming attention backward (S = 300 > 256 keys) takes no mask_bits: the dense phase masks and the "
                                "align-map gradient stay at 256 keys")
        with pytest.raises(NotImplementedError) as e:
            ag._bert_layer_forward(None, x, None, a, 1e-12, 0.0, 0.0, {"_align": (torch.zeros(1, 100, 200), 100, {})}, [],
                                   key_mask=torch.ones(1, 300))
        assert str(e.value) == ("the streaming attention backward (S = 300 > 256 keys) takes no align map: the dense phase masks and the "
                                "align-map gradient stay at 256 keys")
        for kw in (dict(mask_bits=bits), dict(key_mask=torch.ones(1, 300), align_map=torch.zeros(1, 100, 200), align_t=100)):
            with pytest.raises(NotImplementedError) as e:
                hip_layers.layer_forward_train({}, x.detach(), a, 1e-12, long_backward=True, **kw)
            assert str(e.value) == "layer_forward_train: no mask_bits and no align map above 256 keys (long_backward)"
        assert len(names) == 16
    finally:
        ag.set_long_backward(False)


def test_run_scripts_flag():
    import run_PMR_ModCR as pmr
    args = pmr.get_args(["--modcr_long_align"])
    assert args.modcr_long_align and args.modcr_long_backward and not args.modcr_long_dropout
    args = pmr.get_args(["--modcr_long_align", "--modcr_long_dropout"])
    assert args.modcr_long_align and args.modcr_long_backward and args.modcr_long_dropout
    args = pmr.get_args([])
    assert not args.modcr_long_align and not args.modcr_long_backward


def test_sweep_1_online_accumulator_equals_the_direct_sum():
    """the query kernel's align share of D: c <- c * alpha + sum_j e_ij E_ij k_ij per 64-key tile, alpha = exp2(m_old - m_new), rescaled
    with the running max exactly like the row sum and divided by the row sum at the end -- against sum_j A^side_ij E_ij in float64"""
    rs = np.random.RandomState(11)
    for s, t, post in ((257, 200, False), (300, 229, True), (512, 450, True), (258, 257, False)):
        r = s - t
        sc = rs.standard_normal((t, s)) * 6.0
        sc[:, rs.randint(0, s, 40)] -= 10000.0 * np.log2(np.e)             # hidden keys
        sc[3, :] = -10000.0 * np.log2(np.e) + sc[3, :] * 1e-3               # a row hidden everywhere
        g = rs.standard_normal((t, r))
        keep = (rs.uniform(size=(t, s)) >= 0.1) / 0.9 if post else np.ones((t, s))
        e_full = np.zeros((t, s))
        e_full[:, t:] = g
        p = np.exp2(sc - sc.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        direct = (p * keep * e_full).sum(1)
        m = np.full(t, -np.inf)
        lsum, c = np.zeros(t), np.zeros(t)
        for t0 in range(0, s, 64):
            tile = sc[:, t0:t0 + 64]
            mn = np.maximum(m, tile.max(1))
            alpha = np.exp2(m - mn)
            e = np.exp2(tile - mn[:, None])
            lsum = lsum * alpha + e.sum(1)
            sub = (e * keep[:, t0:t0 + 64] * e_full[:, t0:t0 + 64]).sum(1) if t0 + 63 >= t else 0.0    # key tiles below T are skipped
            c = c * alpha + sub
            m = mn
        online = c / lsum
        assert np.abs(online - direct).max() <= 1e-12 * max(1.0, np.abs(direct).max()), (s, t, np.abs(online - direct).max())
