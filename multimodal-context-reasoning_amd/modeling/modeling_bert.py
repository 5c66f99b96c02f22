"""Drop-in for the hot-path classes of the reference's modeling/modeling_bert.py:
CaptionBertSelfAttention (:25-75) and CaptionBertAttention (:78-93), same constructor and forward
signatures and return tuples, arithmetic in libmodcr_hip (fused QKV projection + attention)."""
import torch
from torch import nn

import modcr_hip as mh
from .bert_primitives import BertSelfAttention, BertSelfOutput, additive_to_binary


def split_additive_mask(attention_mask, n, s, l, head_mask=None):
    """The reference's additive attention_mask -> the arguments of hip_forward, as a dict.
    A 0 / -10000 mask without head_mask takes the binary routes: [N,1,1,L] -> key_mask [N,L], [N,1,S,L] -> mask_bits [N,S,LW].
    Anything else -- a soft bias, -5000, -inf, a per-head mask [.,A,.,L], a head_mask -- is added as it is (attn_bias) on the
    general route (modcr_qkv_attn_bias_fwd); the head mask goes with it.  The check costs one reduction and one host read, and is
    paid only by the reference-signature forward()s: the encoders' hip_forward hot path takes 0/1 masks and never comes here."""
    if attention_mask.dim() != 4:
        raise ValueError("attention_mask must be 4-D, broadcastable to [N,A,S,L], got %s" % (tuple(attention_mask.shape),))
    if head_mask is None and attention_mask.shape[1] == 1 and mh.additive_mask_is_binary(attention_mask):
        if attention_mask.shape[2] == 1:
            return dict(key_mask=additive_to_binary(attention_mask.reshape(n, l)))
        return dict(mask_bits=mh.pack_mask_bits(additive_to_binary(attention_mask.reshape(n, s, l))))
    return dict(attn_bias=attention_mask, head_mask=head_mask)


class CaptionBertSelfAttention(BertSelfAttention):
    def __init__(self, config):
        super(CaptionBertSelfAttention, self).__init__(config)
        self.output_attentions = config.output_attentions
        # training mode: the probabilities this module returns (and the align map summed from them) are the ones AFTER nn.Dropout,
        # as in the reference (modeling_bert.py:69-74 applies self.dropout before building `outputs`); False = the un-dropped ones
        self.side_post_dropout = bool(getattr(config, "modcr_align_map_post_dropout", True))

    def hip_forward(self, x, key_mask=None, mask_bits=None, hist=None, chunk_id=None, want_probs=False,
                    align_map=None, align_t=0, workspace=None, out=None, attn_bias=None, head_mask=None, row_start=None):
        """attn_bias / head_mask (instead of key_mask / mask_bits): an additive float mask broadcastable to [N,A,S,L] and a
        per-head multiplier of the probabilities, mh.qkv_attn's general route.  row_start: x and out are [N,S,H] buffers in the
        live-row layout (mh.LiveRows); the attention-dropout counters are those of the dense call."""
        w, b = self.packed_qkv(x.dtype)
        drop, wide = None, False
        if self.training and self.dropout.p > 0.0:      # nn.Dropout on the probabilities (modeling_bert.py:69), training mode
            n, s, h = x.shape
            l = s + (0 if hist is None else hist.shape[1])
            # every route carries the mask for P + S <= 256 (bf16 tile / older kernels, the exact-fp32 route); a probabilities output
            # under dropout is the post-dropout one, as the reference returns it (modeling_bert.py:69-74) -- on shapes the bf16 tile
            # kernels do not serve, mh.qkv_attn runs that call on the exact-fp32 route.  What the library does not offer is an error,
            # not a silently un-dropped forward:
            # (above 256 keys: only with hip_autograd.set_long_backward(True, dropout=True), on the attn_bias route under the wide
            # counter layout -- a binary key mask is folded into a 0 / -10000 bias; dense phase masks stay at 256 keys)
            wide = l > 256
            if wide:
                from . import hip_autograd
                if not hip_autograd.LONG_DROPOUT or l > mh.ATTN_DROPOUT_WIDE_MAX_KEYS or mask_bits is not None or row_start is not None:
                    raise NotImplementedError("attention-probability dropout: P + S = %d exceeds the 256 keys the attention kernels take" % l)
                if key_mask is not None:
                    if attn_bias is not None:
                        raise ValueError("hip_forward: attn_bias replaces key_mask")
                    attn_bias, key_mask = mh.fold_key_mask(key_mask), None
                if attn_bias is None and head_mask is None:
                    attn_bias = torch.zeros((1, 1, 1, l), dtype=torch.float32, device=x.device)
            if want_probs and not self.side_post_dropout:
                raise NotImplementedError("a probabilities output in training mode is the post-dropout one (modeling_bert.py:69-74); "
                                          "config.modcr_align_map_post_dropout=False offers the un-dropped align map only")
            seed, off = mh.DROPOUT.take(n * self.num_attention_heads * s * l)
            drop = (float(self.dropout.p), seed, off)
        return mh.qkv_attn(x, w, b, key_mask=key_mask, mask_bits=mask_bits, hist=hist, chunk_id=chunk_id,
                           want_probs=want_probs, align_map=align_map, align_t=align_t,
                           num_heads=self.num_attention_heads, workspace=workspace, out=out, attn_dropout=drop,
                           side_post_dropout=self.side_post_dropout and drop is not None and (want_probs or align_map is not None),
                           attn_bias=attn_bias, head_mask=head_mask, **({} if row_start is None else {"row_start": row_start}),
                           **({"wide_dropout": True} if wide else {}))

    def forward(self, hidden_states, attention_mask, head_mask=None, history_state=None):
        n, s, _ = hidden_states.shape
        l = s + (0 if history_state is None else history_state.shape[1])
        ctx, probs = self.hip_forward(hidden_states, hist=history_state, want_probs=self.output_attentions,
                                      **split_additive_mask(attention_mask, n, s, l, head_mask))
        return (ctx, probs) if self.output_attentions else (ctx,)


class CaptionBertAttention(nn.Module):
    def __init__(self, config):
        super(CaptionBertAttention, self).__init__()
        self.self = CaptionBertSelfAttention(config)
        self.output = BertSelfOutput(config)

    def forward(self, input_tensor, attention_mask, head_mask=None, history_state=None):
        self_outputs = self.self(input_tensor, attention_mask, head_mask, history_state)
        attention_output = self.output(self_outputs[0], input_tensor)
        return (attention_output,) + self_outputs[1:]
