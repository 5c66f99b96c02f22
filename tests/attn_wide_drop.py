"""Host restatement of the attention-probability dropout mask of csrc/attn_common.h with the counter's row stride as a parameter:
helpers.attn_drop_keep_torch is the stride-256 layout (every call of at most 256 keys); a call of more than 256 keys runs the wide
layout, stride 512.  Everything else -- l4, the word index, the multipliers, the fold, the key, the threshold -- is the same."""
import torch

import helpers as H

M32 = 0xffffffff
WIDE_STRIDE = 512


def stride_of(keys):
    """attn_drop_stride(L): 256 up to 256 keys, 512 above"""
    return WIDE_STRIDE if keys > 256 else 256


def counters(seq, heads, head, query, stride):
    """the four 32-bit counters (l4 = 0..3) of one probability row"""
    row = (seq * heads + head) * stride + query
    return [(row * 4 + l4) & M32 for l4 in range(4)]


def keep(seq_ids, heads, s, p, seed, offset, stride, device="cpu", keys=None):
    """keep[i, head, query, key] (float 0 / 1), row = (n * A + head) * stride + query: helpers.attn_drop_keep_torch with the stride"""
    keys = s if keys is None else keys
    key64 = (seed + offset * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    k = key64 - 2 ** 64 if key64 >= 2 ** 63 else key64
    thr = min(max(int(p * 65536 + 0.5), 1), 65535) - 32768

    def fold(a, c):
        prod = a * c + k                        # int64 arithmetic wraps mod 2^64, as the 64-bit multiply-add does
        return (prod & M32) ^ ((prod >> 32) & M32)

    n_ = torch.as_tensor(list(seq_ids), dtype=torch.int64, device=device).view(-1, 1, 1, 1)
    a_ = torch.arange(heads, dtype=torch.int64, device=device).view(1, -1, 1, 1)
    q_ = torch.arange(s, dtype=torch.int64, device=device).view(1, 1, -1, 1)
    l4_ = torch.arange(4, dtype=torch.int64, device=device).view(1, 1, 1, -1)
    row = (n_ * heads + a_) * stride + q_
    assert int(row.max()) * 4 + 3 <= M32, "the counter is 32 bits wide"
    cm = ((row * 4 + l4_) * 0x9E3779B1) & M32
    base = fold(cm, 0x85EBCA6B)                                       # [n, heads, s, 4]
    key_ = torch.arange(keys, dtype=torch.int64, device=device)
    jj = 2 * (key_ >> 4) + ((key_ >> 1) & 1)
    cs = torch.tensor([H.attn_drop_const(int(j)) for j in jj.tolist()], dtype=torch.int64, device=device)
    w = fold(base[..., (key_ >> 2) & 3], cs)                          # [n, heads, s, keys]
    f = (w >> ((key_ & 1) * 16)) & 0xffff
    f = torch.where(f >= 32768, f - 65536, f)
    return (f >= thr).to(torch.float32)


def keep_of_call(n, heads, s, prefix, drop, device="cpu"):
    """the mask a call of n sequences, s queries and prefix + s keys runs under: drop = (p, seed, offset)"""
    p, seed, off = drop
    return keep(range(n), heads, s, p, seed, off, stride_of(prefix + s), device, keys=prefix + s)
