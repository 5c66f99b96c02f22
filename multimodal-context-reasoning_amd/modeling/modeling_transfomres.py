"""Drop-in for the hot-path classes of the reference's modeling/modeling_transfomres.py (sic):
CaptionBertLayer (:471-502), CaptionBertEncoder (:504-562) and BertImgModel (:564-727) -- the
global_enc of ModCR.  Same constructor/forward signatures and positional return tuples."""
import torch
from torch import nn

import modcr_hip as mh
from .bert_primitives import (BertEmbeddings, BertIntermediate, BertOutput, BertPooler, BertPreTrainedModel,
                              EncoderOutputs, PackCache, additive_to_binary, compute_dtype, packed_linear,
                              packed_ln, _pad64)
from .hip_layers import Workspace
from .modeling_bert import CaptionBertAttention, split_additive_mask


FFN_SPLIT = 1      # tools may raise it for an A/B run: FFN row chunks per layer
PACK_SHORT = 64    # sequences of at most this many rows are packed several to an attention row block (0 = off)
# The frozen encoders' internal route (Abstract_Specific -> ChunkAlign -> the two encoder classes, when the batch carries
# mh.LiveRows tables) runs every layer over the LIVE rows only: padded image-region rows are keys that every mask hides and
# queries that nobody reads, about a quarter of all rows of a PMR batch.  Live rows carry the padded route's values bit for bit
# (same kernels, same operands, the dropout counters of their padded positions).  The reference-signature forward()s without
# `live_rows` compute and return every row as before.  Tools and tests clear the switch for an A/B run.
LIVE_ROWS = True


def live_attn_supported(n, s, h, a, attn_p, modes, align_t=0, chunk_t=0):
    """True when modcr_qkv_attn_rows_fwd serves the attention calls of a pass over sequences of s rows: modes = the subset of
    (1 key mask, 2 dense mask, 3 dense mask + chunk ids + align map) the pass launches"""
    for mode in modes:
        r = mh.qkv_attn_route(n, s, 0, h, a, dense=mode >= 2, chunk_t=chunk_t if mode == 3 else 0, align_t=align_t if mode == 3 else 0,
                              attn_p=attn_p, flags=mh.ATTN_SIDE_POST_DROPOUT if (mode == 3 and attn_p > 0.0) else 0, rows=True)
        if r.rc != 0:
            return False
    return True


def live_buffers(lay, h, dtype, device):
    """(x, ctx) for a pass over the live-row layout `lay`: two [capacity, H] buffers (the padded size, so that the allocator sees the
    same sizes every step) of which the first lay.m_launch rows are used.  x is for the embedding passes to fill (embed_live); ctx
    is the layers' attention output buffer, its filler rows zeroed once."""
    x = torch.empty((lay.capacity, h), dtype=dtype, device=device)
    ctx = torch.empty_like(x)
    if lay.m_launch > lay.m_live:
        ctx[lay.m_live:lay.m_launch].zero_()
    return x, ctx


class CaptionBertLayer(nn.Module):
    def __init__(self, config):
        super(CaptionBertLayer, self).__init__()
        self.attention = CaptionBertAttention(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)

    def hip_forward(self, x, key_mask=None, mask_bits=None, hist=None, chunk_id=None, want_probs=False,
                    align_map=None, align_t=0, ws=None, out_rows=None, seq_len=None, attn_bias=None, head_mask=None):
        """attn_bias / head_mask: CaptionBertSelfAttention.hip_forward's general route (instead of key_mask / mask_bits).
        out_rows = k (opt-in, the LAST layer of a frozen pass whose caller consumes only the first k rows of every sequence:
        config.modcr_last_layer_rows): attention runs over all rows (keys and values of every row are needed), the token-wise
        blocks behind it -- BertSelfOutput, BertIntermediate, BertOutput -- only over rows 0..k-1; returns [N,k,H].  seq_len: the
        sequence length when x is a packed view of several short sequences per row block."""
        ws = ws or Workspace()
        n, s, h = x.shape
        general = attn_bias is not None or head_mask is not None
        need = (mh.lib().modcr_qkv_attn_bias_workspace if general else mh.lib().modcr_qkv_attn_workspace)(
            n, s, 0 if hist is None else hist.shape[1], h, mh.dt_of(x))
        ctx, probs = self.attention.self.hip_forward(x, key_mask, mask_bits, hist, chunk_id, want_probs, align_map,
                                                     align_t, ws.get("attn", need, x.device) if need else None,
                                                     attn_bias=attn_bias, head_mask=head_mask)
        if out_rows is not None:
            sl = seq_len or s
            if out_rows < sl:
                ctx = ctx.reshape(-1, sl, h)[:, :out_rows].contiguous()
                x = x.reshape(-1, sl, h)[:, :out_rows].contiguous()
                n, s = ctx.shape[0], out_rows
            elif seq_len:
                ctx, x = ctx.reshape(-1, sl, h), x.reshape(-1, sl, h)
                n, s = ctx.shape[0], sl
        pre = ws.get("preln", n * s * h * 4, x.device)
        a = self.attention.output(ctx, x, pre)
        if FFN_SPLIT <= 1 or (n * s) % (8 * FFN_SPLIT):
            y = self.output(self.intermediate(a), a, pre)
        else:
            # the FFN in row chunks: BertIntermediate's [rows, 4H] output of one chunk is read back by BertOutput while
            # it still sits in the 256 MB Infinity Cache (283 MB at 46080 rows do not)
            m, rows = n * s, (n * s) // FFN_SPLIT
            a2 = a.reshape(m, h)
            y = torch.empty_like(a2)
            for c in range(FFN_SPLIT):
                ac = a2[c * rows:(c + 1) * rows]
                self.output(self.intermediate(ac), ac, pre, out=y[c * rows:(c + 1) * rows])
            y = y.view(n, s, h)
        return y, probs

    def hip_forward_live(self, x, ctx, lay, passes):
        """One layer over a live-row layout (mh.LiveLayout `lay`).  x, ctx: [capacity, H] buffers (compact_rows); passes: one
        (first row, sequences, rows per sequence, row_start table, attention keywords) per attention launch.  The token-wise
        blocks run once over the first lay.m_launch rows, with the hidden-dropout counters of the padded buffer.  Returns the new
        [capacity, H] buffer."""
        h = x.shape[1]
        for r0, n, s, row_start, kw in passes:
            self.attention.self.hip_forward(x[r0:r0 + n * s].view(n, s, h), out=ctx[r0:r0 + n * s].view(n, s, h), row_start=row_start, **kw)
        m = lay.m_launch
        live = (lay.row_id, lay.capacity)
        a = self.attention.output(ctx[:m], x[:m], live=live)
        y = torch.empty_like(x)
        self.output(self.intermediate(a), a, out=y[:m], live=live)
        return y

    def forward(self, hidden_states, attention_mask, head_mask=None, history_state=None):
        n, s, _ = hidden_states.shape
        l = s + (0 if history_state is None else history_state.shape[1])
        want = self.attention.self.output_attentions
        y, probs = self.hip_forward(hidden_states, hist=history_state, want_probs=want,
                                    **split_additive_mask(attention_mask, n, s, l, head_mask))
        return (y, probs) if want else (y,)

    def attention_cal(self, hidden_states, attention_mask, head_mask=None, history_state=None):
        return self.attention(hidden_states, attention_mask, head_mask, history_state)[0]

    def forward_ffn(self, attention_output):
        return self.output(self.intermediate(attention_output), attention_output)


class CaptionBertEncoder(nn.Module):
    def __init__(self, config):
        super(CaptionBertEncoder, self).__init__()
        self.output_attentions = config.output_attentions
        self.output_hidden_states = config.output_hidden_states
        self.materialize = getattr(config, "modcr_materialize_attentions", False)
        self.layer = nn.ModuleList([CaptionBertLayer(config) for _ in range(config.num_hidden_layers)])

    def hip_forward(self, x, key_mask, encoder_history_states=None, ws=None, last_rows=None, dense_bits=None):
        """last_rows = k (opt-in): the caller reads only rows 0..k-1 of the final hidden states (ModCR: the text rows, or the
        [CLS] row of the image-only pass) -- the last layer's token-wise blocks skip the other rows and the result is [N,k,H]."""
        ws = ws or Workspace()
        all_hidden, all_att = (), ()
        want = self.output_attentions and self.materialize
        if want or self.output_hidden_states or encoder_history_states is not None:
            last_rows = None
        # Short sequences (the image-only pass: S = 1 + R rows, modeling_ensemble.py:466-471) packed k to an attention row block
        # under a block-diagonal mask, so that the 192- / 256-token tile kernels are filled (S = 37 alone runs the older kernel at
        # a third of their rate; every other op of a layer is row-wise and does not see the packing).
        n, s, h = x.shape
        pack_k, bits = 1, None
        if dense_bits is not None:
            # a per-(query, key) mask (3-D attention_mask, modeling_transfomres.py:629-630): every layer on the dense-mask kernels
            if encoder_history_states is not None:
                raise NotImplementedError("a 3-D attention_mask together with encoder_history_states")
            for i, layer in enumerate(self.layer):
                if self.output_hidden_states:
                    all_hidden = all_hidden + (x,)
                x, probs = layer.hip_forward(x, mask_bits=dense_bits, want_probs=want, ws=ws)
                if self.output_attentions:
                    all_att = all_att + (probs,)
            if self.output_hidden_states:
                all_hidden = all_hidden + (x,)
            outputs = (x,)
            if self.output_hidden_states:
                outputs = outputs + (all_hidden,)
            if self.output_attentions:
                outputs = outputs + (all_att,)
            return outputs
        if (PACK_SHORT and x.dtype == torch.bfloat16 and not want and encoder_history_states is None and not self.output_hidden_states
                and key_mask is not None and s <= PACK_SHORT):
            pack_k = mh.pack_factor(n, s)
            if pack_k > 1 and pack_k * s > 64:
                bits = mh.build_packed_mask(key_mask, pack_k)
                x = x.view(n // pack_k, pack_k * s, h)
            else:
                pack_k = 1
        for i, layer in enumerate(self.layer):
            if self.output_hidden_states:
                all_hidden = all_hidden + (x,)
            hist = None if encoder_history_states is None else encoder_history_states[i]
            last = i == len(self.layer) - 1
            if pack_k > 1:
                if last and last_rows is not None:
                    x, probs = layer.hip_forward(x, mask_bits=bits, ws=ws, out_rows=last_rows, seq_len=s)
                else:
                    x, probs = layer.hip_forward(x, mask_bits=bits, ws=ws)
                    if last:
                        x = x.view(n, s, h)
                if self.output_attentions:
                    all_att = all_att + (None,)
                continue
            x, probs = layer.hip_forward(x, key_mask=key_mask, hist=hist, want_probs=want, ws=ws,
                                         out_rows=last_rows if last else None)
            if self.output_attentions:
                all_att = all_att + (probs,)
        if self.output_hidden_states:
            all_hidden = all_hidden + (x,)
        outputs = (x,)
        if self.output_hidden_states:
            outputs = outputs + (all_hidden,)
        if self.output_attentions:
            outputs = outputs + (all_att,)
        return outputs

    def hip_forward_live(self, xc, ctx, n, key_mask, lay):
        """hip_forward's key-mask route over the live rows of one pass: xc, ctx [capacity, H] (live_buffers, xc filled by embed_live)
        -> the compact [capacity, H] rows of the last layer (rows lay.row_start[n] + j = row j of sequence n)"""
        s = lay.seq_len
        for layer in self.layer:
            xc = layer.hip_forward_live(xc, ctx, lay, [(0, n, s, lay.row_start, {"key_mask": key_mask})])
        return xc

    def hip_forward_pair_live(self, xc, ctx, n, s1, s2, mask1, mask2, live):
        """hip_forward_pair over the live rows of both passes (live.pair; xc, ctx: live_buffers, xc filled by embed_live): returns
        the compact rows"""
        lay = live.pair
        m1 = live.full.m_live
        passes = [(0, n, s1, live.full.row_start, {"key_mask": mask1}), (m1, n, s2, live.img.row_start, {"key_mask": mask2})]
        for layer in self.layer:
            xc = layer.hip_forward_live(xc, ctx, lay, passes)
        return xc

    def hip_forward_pair(self, rows, n, s1, s2, mask1, mask2, ws=None):
        """Two passes of the SAME encoder over different sequences (ModCR: the full [text | regions] pass of
        calec and the image-only [CLS | regions] pass of Abstract_Specific, modeling_ensemble.py:466-471) as one
        batch: `rows` [n*s1 + n*s2, H] holds both; attention runs per pass (two launches per layer), the
        token-wise blocks (BertSelfOutput, BertIntermediate, BertOutput) once over all rows -- at N=256 that is
        71936 rows = 2.9 rounds of the 192x384 GEMM tiles instead of 1.9 + 2 half-empty ones."""
        ws = ws or Workspace()
        h = rows.shape[1]
        m1 = n * s1
        ctx = torch.empty_like(rows)
        for layer in self.layer:
            xa, xb = rows[:m1].view(n, s1, h), rows[m1:].view(n, s2, h)
            layer.attention.self.hip_forward(xa, mask1, out=ctx[:m1].view(n, s1, h))
            layer.attention.self.hip_forward(xb, mask2, out=ctx[m1:].view(n, s2, h))
            pre = ws.get("preln", rows.shape[0] * h * 4, rows.device)
            a = layer.attention.output(ctx, rows, pre)
            rows = layer.output(layer.intermediate(a), a, pre)
        return rows[:m1].view(n, s1, h), rows[m1:].view(n, s2, h)

    def forward(self, hidden_states, attention_mask, head_mask=None, encoder_history_states=None):
        n, s, _ = hidden_states.shape
        p = 0 if not encoder_history_states else encoder_history_states[0].shape[1]
        if head_mask is not None and not (torch.is_tensor(head_mask) or len(head_mask) == len(self.layer)):
            raise ValueError("head_mask: one entry per layer (%d), got %d" % (len(self.layer), len(head_mask)))
        if head_mask is None or all(hm is None for hm in head_mask):
            m = split_additive_mask(attention_mask, n, s, s + p)
            if "key_mask" in m:                                 # the binary key mask: today's route, all its packing included
                return self.hip_forward(hidden_states, m["key_mask"], encoder_history_states)
            if "mask_bits" in m:
                raise NotImplementedError("global_enc always uses the broadcast padding mask (modeling_transfomres.py:628-641)")
            head_mask = [None] * len(self.layer)
        # a non-binary additive mask and / or a head mask per layer (head_mask[i], as the reference indexes it): layer by layer on
        # the general route, outputs laid out as hip_forward's
        want = self.output_attentions and self.materialize
        ws = Workspace()
        x, all_hidden, all_att = hidden_states, (), ()
        for i, layer in enumerate(self.layer):
            if self.output_hidden_states:
                all_hidden = all_hidden + (x,)
            hist = None if encoder_history_states is None else encoder_history_states[i]
            x, probs = layer.hip_forward(x, hist=hist, want_probs=want, ws=ws, attn_bias=attention_mask, head_mask=head_mask[i])
            if self.output_attentions:
                all_att = all_att + (probs,)
        if self.output_hidden_states:
            all_hidden = all_hidden + (x,)
        outputs = (x,)
        if self.output_hidden_states:
            outputs = outputs + (all_hidden,)
        if self.output_attentions:
            outputs = outputs + (all_att,)
        return outputs


class ImgEmbedMixin(object):
    """img_embedding + LayerNorm of the region features (modeling_transfomres.py:676-681), written
    behind the text rows of each sequence (the torch.cat at :684)."""

    _cast_cache = None      # (img_feats tensor, its version, kp, dtype, epoch) -> padded copy in the storage dtype, shared by all encoders
    _epoch = 0              # bumped by every Abstract_Specific.forward: nothing computed in one model call is re-used by the next

    def region_rows(self, img_feats, dt, reg=None):
        """LayerNorm(img_embedding(img_feats)) as [N*R, H] rows in the storage dtype `dt` (modeling_transfomres.py:676-680), before
        the dropout.  One ModCR step embeds the SAME region features three times (global_enc full pass, global_enc image-only pass,
        seq_enc: modeling_ensemble.py:466-471, v10:896-907).  The padded storage-dtype copy of the features is shared by
        all three, and an encoder whose weights have not changed re-uses its LayerNorm-ed region rows for a second call
        on the same tensor (global_enc's two passes).  Validity = the very same tensor object at the same version (a
        reference is held, so its memory cannot be recycled under the cache) within ONE forward of the whole model
        (`_epoch`): a common subexpression of a step is computed once, nothing is carried from step to step.
        reg (mh.LiveRows.reg): the cast, the GEMM and the LayerNorm run over the layout's region rows only -- [reg.m_launch, H] rows
        back to back, row reg.row_start[n] + j = region j of sequence n (the same values: every kernel here works row by row)."""
        n, r, d = img_feats.shape
        if not self.use_img_layernorm:
            raise NotImplementedError("use_img_layernorm=False: the Oscar checkpoints ModCR loads set it (run_PMR_ModCR.py:720)")
        w, b = packed_linear(self._cache, ("img", dt), self.img_embedding, dt)
        g, be = packed_ln(self._cache, "imgln", self.LayerNorm)
        kp = _pad64(d) if dt == torch.bfloat16 else d
        rc = getattr(self, "_region_cache", None)
        ep = ImgEmbedMixin._epoch
        if (rc is not None and rc[0] is img_feats and rc[1] == img_feats._version and rc[2] is w and rc[3] is g and rc[4].dtype == dt
                and rc[5] == ep and rc[6] is reg and not torch.is_grad_enabled()):
            return rc[4]
        cc = ImgEmbedMixin._cast_cache
        if cc is not None and cc[0] is img_feats and cc[1] == img_feats._version and cc[2] == kp and cc[3] == dt and cc[5] == ep and cc[6] is reg:
            src = cc[4]
        else:
            if reg is not None:
                src = mh.cast_pad_rows(img_feats, kp, reg.row_id)                                 # live region rows only (bf16)
            else:
                src = mh.cast_pad(img_feats, kp, mh.BF16 if dt == torch.bfloat16 else mh.F32)     # fp32 [N*R,2054] -> dtype [N*R,Kp]
            ImgEmbedMixin._cast_cache = (img_feats, img_feats._version, kp, dt, src, ep, reg)
        pre = mh.linear(src, w, b, out_dtype=mh.F32)
        rows = mh.layernorm(pre, g, be, self.config.img_layer_norm_eps, out_dtype=mh.BF16 if dt == torch.bfloat16 else mh.F32)
        if not torch.is_grad_enabled():
            self._region_cache = (img_feats, img_feats._version, w, g, rows, ep, reg)
        return rows

    def embed_regions(self, img_feats, out, t, dropout=None):
        """the region rows behind the text rows of each sequence of `out` [N, T+R, H] (the torch.cat at :684).
        dropout = (p, seed, offset): self.dropout of the reference (:681) rides on the pass that places the rows
        (counters = flat indices of `out`; BertEmbeddings.forward(dropout=) covers the text rows under the same (seed, offset))."""
        return mh.rows_scatter_dropout(self.region_rows(img_feats, out.dtype), out, t, dropout)

    def live_rows_usable(self, live_rows, n, t, r, device):
        """what both encoder classes ask before a frozen pass runs over live rows: the switch, tables made for this batch shape and
        device, bf16, a plain frozen pass (nothing materialised, no row chunks, every last-layer row wanted)"""
        enc, cfg = self.encoder, self.config
        return not (not LIVE_ROWS or live_rows is None or not live_rows.matches(n, t, r, device) or compute_dtype(cfg) != torch.bfloat16
                    or torch.is_grad_enabled() and getattr(self, "trainable", False) or FFN_SPLIT > 1
                    or enc.output_hidden_states or (enc.output_attentions and enc.materialize) or getattr(cfg, "modcr_last_layer_rows", False))

    def embed_live(self, input_ids, token_type_ids, position_ids, img_feats, x, lay, live, dropout=None, filler=True):
        """embeddings + embed_regions of one pass written straight into the live-row layout `lay` (live.full or live.img of the
        mh.LiveRows `live`): x [>= lay.m_launch, H] gets the layout's rows back to back and zero filler rows.  dropout = (p, seed,
        offset) of the ONE dropout over the padded [N, lay.seq_len, H] buffer: every row takes the counters of its padded position,
        so x holds what the padded passes followed by a gather of the live rows would.  filler=False: only the lay.m_live live rows
        are written (forward_pair: another pass's rows follow at once)."""
        t = input_ids.shape[1]
        m = lay.m_launch if filler else lay.m_live
        self.embeddings(input_ids, token_type_ids, position_ids, out=x, dropout=dropout, row_start=lay.row_start, seq_stride=lay.seq_len)
        mh.rows_place_dropout(self.region_rows(img_feats, x.dtype, live.reg), x[:m], lay.row_id[:m], live.r, lay.seq_len, t, dropout,
                              src_start=live.reg.row_start)
        return x


class BertImgModel(BertPreTrainedModel, ImgEmbedMixin):
    """Expand from BertModel to handle image region features as input (global_enc)."""

    def __init__(self, config):
        super(BertImgModel, self).__init__(config)
        self.embeddings = BertEmbeddings(config)
        self.encoder = CaptionBertEncoder(config)
        self.pooler = BertPooler(config)
        self.img_dim = config.img_feature_dim
        self.img_feature_type = config.img_feature_type
        self.use_img_layernorm = getattr(config, "use_img_layernorm", None)
        if config.img_feature_type not in ("frcnn", "faster_r-cnn", None):
            raise NotImplementedError("img_feature_type=%r (ModCR uses region features)" % (config.img_feature_type,))
        self.img_embedding = nn.Linear(self.img_dim, self.config.hidden_size, bias=True)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        if self.use_img_layernorm:
            self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.img_layer_norm_eps)
        self._cache = PackCache()
        self._ws = Workspace()
        self.init_weights()

    def live_route(self, live_rows, n, t, r, device, passes):
        """the mh.LiveRows to run this frozen pass over, or None (the padded route): live_rows_usable and attention shapes
        modcr_qkv_attn_rows_fwd serves.  passes: the sequence lengths whose key-mask attention the pass launches"""
        cfg = self.config
        if not self.live_rows_usable(live_rows, n, t, r, device):
            return None
        sa = self.encoder.layer[0].attention.self
        attn_p = float(sa.dropout.p) if sa.training else 0.0
        if not all(s > PACK_SHORT and live_attn_supported(n, s, cfg.hidden_size, cfg.num_attention_heads, attn_p, (1,)) for s in passes):
            return None
        return live_rows

    def forward_pair(self, input_ids, token_type_ids, attention_mask, img_feats, img_attention_mask, position_ids=None, live_rows=None):
        """forward(input_ids, token_type_ids, attention_mask, img_feats=...) AND forward(input_ids[:, :1],
        attention_mask=img_attention_mask, img_feats=...) (the image-only call of modeling_ensemble.py:466-471) in
        one batch; returns the two output tuples (sequence_output, pooled_output).  The region embeddings are
        computed once and copied behind the [CLS] row of the image-only sequences."""
        n, t = input_ids.shape
        r = img_feats.shape[1]
        h = self.config.hidden_size
        dt = compute_dtype(self.config)
        s1, s2 = t + r, 1 + r
        da = db = None
        if self.training and self.dropout.p > 0.0:          # BertEmbeddings.dropout + self.dropout (:681) of each of the two calls
            da = (self.dropout.p,) + tuple(mh.DROPOUT.take(n * s1 * h))
            db = (self.dropout.p,) + tuple(mh.DROPOUT.take(n * s2 * h))
        live = self.live_route(live_rows, n, t, r, input_ids.device, (s1, s2))
        if live is not None:
            # live rows only, embedded in place; what the callers read comes back dense: the text rows of the full pass [N,T,H],
            # [CLS] of the other [N,1,H]
            xc, ctx = live_buffers(live.pair, h, dt, input_ids.device)
            m1, m2 = live.full.m_live, live.img.m_live
            self.embed_live(input_ids, token_type_ids, position_ids, img_feats, xc, live.full, live, da, filler=False)
            self.embed_live(input_ids[:, :1].contiguous(), None, None, img_feats, xc[m1:], live.img, live, db, filler=False)
            if live.pair.m_launch > m1 + m2:
                xc[m1 + m2:live.pair.m_launch].zero_()
            yc = self.encoder.hip_forward_pair_live(xc, ctx, n, s1, s2, attention_mask.to(torch.float32), img_attention_mask.to(torch.float32), live)
            ya = mh.rows_take(yc, live.pair.take[t]).view(n, t, h)
            yb = mh.rows_take(yc, live.pair.take["img"]).view(n, 1, h)
            att = ((None,) * len(self.encoder.layer),) if self.encoder.output_attentions else ()
            return (ya, self.pooler(ya)) + att, (yb, self.pooler(yb)) + att
        rows = torch.empty((n * s1 + n * s2, h), dtype=dt, device=input_ids.device)
        xa, xb = rows[:n * s1].view(n, s1, h), rows[n * s1:].view(n, s2, h)
        self.embeddings(input_ids, token_type_ids, position_ids, out=xa, dropout=da)
        self.embed_regions(img_feats, xa, t, dropout=da)
        self.embeddings(input_ids[:, :1].contiguous(), None, None, out=xb, dropout=db)
        self.embed_regions(img_feats, xb, 1, dropout=db)     # (the rows of the call above: region_rows' cache, or recomputed)
        ya, yb = self.encoder.hip_forward_pair(rows, n, s1, s2, attention_mask.to(torch.float32),
                                               img_attention_mask.to(torch.float32), self._ws)
        att = ((None,) * len(self.encoder.layer),) if self.encoder.output_attentions else ()
        return (ya, self.pooler(ya)) + att, (yb, self.pooler(yb)) + att

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, position_ids=None, head_mask=None,
                img_feats=None, encoder_history_states=None, modcr_last_rows=None, live_rows=None):
        """modcr_last_rows = k (not in the reference's signature; frozen route only): sequence_output is [N,k,H], the first k rows of
        every sequence -- the last layer computes nothing behind its attention for the rows the caller does not read.
        live_rows (not in the reference's signature; this project's own callers on the frozen route): the batch's mh.LiveRows --
        the layers run over the live rows only and sequence_output is [N,T,H], the text rows (T = 1: the image-only call's [CLS])."""
        if head_mask is not None:
            raise NotImplementedError("head_mask is never set on the ModCR path")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        dense_bits = None
        if attention_mask.dim() == 3:
            # [N, S, S] 0/1 per (query, key): the reference extends it to [N, 1, S, S] and adds (1 - m) * -10000
            # (modeling_transfomres.py:629-630); ModCR itself never passes one to global_enc.  Frozen route.
            if getattr(self, "trainable", False) and torch.is_grad_enabled():
                raise NotImplementedError("3-D attention_mask on the trainable global_enc route")
            dense_bits = mh.pack_mask_bits(attention_mask.to(torch.float32))
        elif attention_mask.dim() != 2:
            raise NotImplementedError
        if encoder_history_states:
            assert img_feats is None, "Cannot take image features while using encoder history states"
        if getattr(self, "trainable", False) and torch.is_grad_enabled() and not encoder_history_states:
            # encoder with gradients (v10:1016-1084 runs it outside no_grad): same kernels behind autograd Functions
            from . import trainable_encoders
            seq, pooled = trainable_encoders.global_encoder(self, input_ids, token_type_ids, attention_mask, position_ids,
                                                            img_feats)
            att = ((None,) * len(self.encoder.layer),) if self.encoder.output_attentions else ()
            return (seq, pooled) + att
        n, t = input_ids.shape
        r = 0 if img_feats is None else img_feats.shape[1]
        dt = compute_dtype(self.config)
        h = self.config.hidden_size
        drop = None
        if self.training and self.dropout.p > 0.0:          # BertEmbeddings.dropout (a_bert:210) and self.dropout (:681): same p,
            drop = (self.dropout.p,) + tuple(mh.DROPOUT.take(n * (t + r) * h))     # one mask over x, applied by the passes that write its rows
        live = None
        if (live_rows is not None and img_feats is not None and dense_bits is None and modcr_last_rows is None and not encoder_history_states
                and live_rows.r == r and t in (live_rows.t, 1)):
            live = self.live_route(live_rows, n, live_rows.t, r, input_ids.device, (t + r,))
        if live is not None:
            lay = live.full if t == live.t else live.img          # (T = 1: both are the same layout)
            xc, ctx = live_buffers(lay, h, dt, input_ids.device)
            self.embed_live(input_ids, token_type_ids, position_ids, img_feats, xc, lay, live, drop)
            yc = self.encoder.hip_forward_live(xc, ctx, n, attention_mask.to(torch.float32), lay)
            sequence_output = mh.rows_take(yc, lay.take[t]).view(n, t, h)
            att = ((None,) * len(self.encoder.layer),) if self.encoder.output_attentions else ()
            return (sequence_output, self.pooler(sequence_output)) + att
        x = torch.empty((n, t + r, h), dtype=dt, device=input_ids.device)
        self.embeddings(input_ids, token_type_ids, position_ids, out=x, dropout=drop)
        if img_feats is not None:
            self.embed_regions(img_feats, x, t, dropout=drop)
        encoder_outputs = self.encoder.hip_forward(x, None if dense_bits is not None else attention_mask.to(torch.float32),
                                                   encoder_history_states, self._ws, last_rows=modcr_last_rows, dense_bits=dense_bits)
        sequence_output = encoder_outputs[0]
        pooled_output = self.pooler(sequence_output)
        return (sequence_output, pooled_output,) + encoder_outputs[1:]
