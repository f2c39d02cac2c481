"""CSATrans assembled around the MI355X attention kernels (the caller side of the hot path).

Mirrors module/csa_trans.py:67-236, module/sbm_model.py, module/base_seq2seq.py:40-114 and
module/components.py with the SAME module attribute names, so the state_dict keys match the
reference's and reference checkpoints load. What changes:

* SBM encoder attention = csa_amd.module.sbm_attn.Attention (fused HIP SBM/dense kernels); the
  per-layer (B,H,N,N) graph/attn maps are not materialised unless ``return_maps=True``
  (the train step discards them, script/train.py:107).
* CSE relation attention = csa_amd.module.disentangled_attn.DisentangledAttn fed the compact
  (B,2,N,N) uint8 relation planes (parent L, sibling T) directly, instead of the reference's
  repeat(4)+cat int64 (B,8,N,N) copies (module/csa_trans.py:206-211).
* Glue (csa_amd/glue.py): Linear (bias gradient kernel), LayerNorm kernels and the decoder's
  MultiheadAttention keep nn's parameters and state_dict keys; they run the decoder's permuted
  sequence-first views on their batch-first memory instead of copying them. Embeddings, dropout,
  GELU and SDPA are stock PyTorch-ROCm, as in the reference.

What has no counterpart in the reference lives elsewhere and is re-exported here: the KV-cached decoding strategies in
csa_amd.decoding (over Embeddings.step, BaseDecoder.step and DecodeCache below), the metrics in csa_amd.metrics.
"""
import copy
import math
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from .data import BOS, UNK
from .glue import LayerNorm, Linear, MultiheadAttention, gelu_dropout, residual_dropout
from .metrics import SummaryMetrics, evaluate  # noqa: F401 (the scorer of what the generators below return)
from .module.disentangled_attn import DisentangledAttn
from .module.sbm_attn import Attention

PAD = 0


def _clones(m, n):
    return nn.ModuleList([copy.deepcopy(m) for _ in range(n)])


class PositionalEncoding(nn.Module):
    """components.py:PositionalEncoding (sinusoidal, buffer `pe`)."""

    def __init__(self, emb_size, max_len=5000):
        super().__init__()
        position = torch.arange(0, max_len).unsqueeze(1)
        div = torch.exp(torch.arange(0, emb_size, 2) * -(math.log(10000.0) / emb_size))
        pe = torch.zeros(max_len, emb_size)
        pe[:, 0::2] = torch.sin(position * div)
        pe[:, 1::2] = torch.cos(position * div)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return x + self.pe[:, : x.size(1)]


class Embeddings(nn.Module):
    """components.py:Embeddings: word embedding (+ positional) -> LayerNorm -> dropout."""

    def __init__(self, hidden_size, vocab_size, dropout=0.1, with_pos=False):
        super().__init__()
        self.word_embeddings = nn.Embedding(vocab_size, hidden_size, padding_idx=0)
        self.pos_emb = PositionalEncoding(hidden_size) if with_pos else None
        self.norm = LayerNorm(hidden_size)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        e = self.word_embeddings(x)
        if self.pos_emb is not None:
            e = self.pos_emb(e)
        return self.dropout(self.norm(e))

    def step(self, x, t):
        """forward() for the single position t: tokens x (B, 1) -> the row forward() gives at index t.
        With t a device counter (1-element int32 tensor) x is the whole (B, T) token buffer and the kernel picks
        column t itself (decode_ops.decode_embed; eval mode only)."""
        if isinstance(t, torch.Tensor):
            from .decode_ops import decode_embed
            return decode_embed(x, t, self).unsqueeze(1)
        e = self.word_embeddings(x)
        if self.pos_emb is not None:
            e = e + self.pos_emb.pe[:, t:t + 1]
        return self.dropout(self.norm(e))


class FeedForward(nn.Module):
    def __init__(self, d_model, dim_feed_forward, dropout=0.1):
        super().__init__()
        self.linear1 = Linear(d_model, dim_feed_forward)
        self.linear2 = Linear(dim_feed_forward, d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        return self.linear2(gelu_dropout(self.linear1(x), self.dropout)), None


class SublayerConnection(nn.Module):
    """Pre-LN residual: x + dropout(sublayer(norm(x)))."""

    def __init__(self, size, dropout):
        super().__init__()
        self.norm = LayerNorm(size)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, sublayer):
        out, w = sublayer(self.norm(x))
        return residual_dropout(x, out, self.dropout), w


class CSE_layer(nn.Module):  # noqa: N801 (reference name)
    def __init__(self, hidden_size, num_heads, dim_feed_forward, dropout):
        super().__init__()
        self.num_heads = num_heads
        self.hidden_size = hidden_size
        self.self_attn = DisentangledAttn(num_heads, hidden_size, dropout)
        self.feed_forward = FeedForward(hidden_size, dim_feed_forward, dropout=dropout)
        self.dropout = nn.Dropout(dropout)
        self.sublayer = _clones(SublayerConnection(hidden_size, dropout), 2)

    def forward(self, src, rel_emb, rel, mask):
        src, _ = self.sublayer[0](src, lambda x: self.self_attn(x, x, x, rel_emb, rel, mask))
        src, _ = self.sublayer[1](src, self.feed_forward)
        return src


class CSE(nn.Module):
    """module/csa_trans.py:180-217 with zero-copy relation planes."""

    def __init__(self, encoder_layer, num_layers, num_heads, hidden_size, dropout=0.2, max_src_len=150):
        super().__init__()
        self.layers = _clones(encoder_layer, num_layers)
        self.num_heads = num_heads
        self.hidden_size = hidden_size
        self.d_k = hidden_size // num_heads
        self.max_src_len = max_src_len
        self.edge_dim = self.d_k
        self.L_q = nn.Embedding(max_src_len, hidden_size)
        self.T_q = nn.Embedding(max_src_len, hidden_size)
        self.f = nn.ReLU()
        self.dropout = nn.Dropout(dropout)
        self.norm = LayerNorm(hidden_size)

    def build_rel_emb(self):
        # the reference's torch.stack([L_q.weight, T_q.weight]), kept as the pair its layers unbind
        return [(self.L_q.weight, self.T_q.weight)]

    def forward(self, data):
        out = data.src_pe_emb
        rel, mask = getattr(data, "rel", None), getattr(data, "rel_mask", None)
        if rel is None or mask is None:
            rel = torch.stack([data.L, data.T], 1)          # (B,2,N,N) uint8: heads 0-3 read L, 4-7 read T
            mask = torch.stack([data.L_mask, data.T_mask], 1)
        elif mask.dtype == torch.bool:  # batch_ops.ast_batch's buffers: no copy (the kernels read bytes)
            mask = mask.view(torch.uint8)
        rel_emb = self.build_rel_emb()
        for layer in self.layers:
            out = layer(out, rel_emb, rel, mask)
        return self.norm(out)


class Transformer(nn.Module):
    """module/sbm_model.py:10-31 pre-LN block around the fused Attention."""

    def __init__(self, config, idx):
        super().__init__()
        self.norm1 = LayerNorm(config["transformer_dim"])
        self.mha = Attention(config, idx, config["full_att"])
        self.dropout1 = nn.Dropout(p=config["dropout_prob"])
        self.norm2 = LayerNorm(config["transformer_dim"])
        self.mlpblock = nn.Sequential(
            Linear(config["transformer_dim"], config["transformer_hidden_dim"]), nn.GELU(),
            nn.Dropout(p=config["dropout_prob"]),
            Linear(config["transformer_hidden_dim"], config["transformer_dim"]), nn.Dropout(p=config["dropout_prob"]))

    def forward(self, X, mask, deliver):
        out, sparsity, graph, attn = self.mha([self.norm1(X), mask, deliver])
        X = residual_dropout(X, out, self.dropout1)  # dropout1(out) + X
        lin1, gelu, drop, lin2, drop2 = self.mlpblock  # Linear, GELU, Dropout, Linear, Dropout
        if gelu.approximate == "none":
            h = lin2(gelu_dropout(lin1(self.norm2(X)), drop))
        else:
            h = lin2(drop(gelu(lin1(self.norm2(X)))))
        X = residual_dropout(X, h, drop2)  # mlpblock(norm2(X)) + X: its last module is the Dropout
        return X, sparsity, graph, attn


class SBM(nn.Module):
    """module/sbm_model.py:34-70."""

    def __init__(self, config, sbm_enc_dim, pe_dim, pegen_dim, use_pegen):
        super().__init__()
        self.num_layers = config["sbm_layers"]
        for idx in range(self.num_layers):
            setattr(self, f"transformer_{idx}", Transformer(config, idx))
        self.norm = LayerNorm(sbm_enc_dim)
        self.out = Linear(sbm_enc_dim, config["out_dim"])
        if use_pegen == "sequential":
            self.pe = PositionalEncoding(sbm_enc_dim, config["max_src_len"])
        else:
            self.pe_expand = Linear(pegen_dim, pe_dim)
        self.use_pegen = use_pegen

    def forward(self, data, src_pe, use_pe):
        mask = data.src_mask
        if use_pe != "sequential":
            pe = self.pe_expand(src_pe)
            X = torch.cat([data.src_emb, pe], dim=-1)
        else:
            pe = None
            X = self.pe(data.src_emb)
        sparsities, graphs, attns = (), [], []
        for idx in range(self.num_layers):
            X, sp, g, a = getattr(self, f"transformer_{idx}")(X, mask, [])
            sparsities += (sp,)
            graphs.append(g)
            attns.append(a)
        X = self.norm(X) * ~mask[:, :, None]
        return self.out(X), sparsities, graphs, attns, pe


class DecoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="gelu"):
        super().__init__()
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.feed_forward = FeedForward(d_model, dim_feedforward, dropout=dropout)
        self.sublayer = _clones(SublayerConnection(d_model, dropout), 3)
        self.dropout3 = nn.Dropout(dropout)

    def forward(self, tgt, memory, tgt_mask=None, memory_key_padding_mask=None):
        tgt, _ = self.sublayer[0](tgt, lambda x: self.self_attn(x, x, x, attn_mask=tgt_mask, need_weights=False))
        tgt, w = self.sublayer[1](tgt, lambda x: self.multihead_attn(
            x, memory, memory, key_padding_mask=memory_key_padding_mask, need_weights=False))
        tgt, _ = self.sublayer[2](tgt, self.feed_forward)
        return tgt, w

    def forward_fused(self, tgt, memory, tgt_pad=None, memory_key_padding_mask=None, mask_mode="own", kv_group=1):
        """forward() on batch-first tensors and MultiheadAttention.forward_fused: tgt (R, T, E), memory (B, S, E) with
        R = B * kv_group, tgt_pad (R, T) uint8 / bool (non-zero = PAD key; the causal mask is implied), the memory mask
        (B, S). The same three sublayers; the kv_group rows of an AST share one memory projection."""
        tgt, _ = self.sublayer[0](tgt, lambda x: (self.self_attn.forward_fused(
            x, key_mask=tgt_pad, causal=True, mask_mode=mask_mode), None))
        memory_kv = self.multihead_attn.project_memory_grad(memory)
        tgt, _ = self.sublayer[1](tgt, lambda x: (self.multihead_attn.forward_fused(
            x, memory_kv=memory_kv, key_mask=memory_key_padding_mask, kv_group=kv_group), None))
        tgt, _ = self.sublayer[2](tgt, self.feed_forward)
        return tgt

    def step(self, x, cache, i, t):
        """forward() in eval mode for the single position t (an int, or the device counter), x (B, 1, E):
        x + sublayer(norm(x)) three times against layer i's slots of a DecodeCache."""
        sl = self.sublayer
        x = x + self.self_attn.step(sl[0].norm(x), cache.self_k[i], cache.self_v[i], t, key_mask=cache.self_mask,
                                    anc=cache.anc)
        x = x + self.multihead_attn.step(sl[1].norm(x), memory_kv=cache.memory_kv[i], key_mask=cache.memory_mask,
                                         kv_group=cache.kv_group)
        return x + self.feed_forward(sl[2].norm(x))[0]


class DecodeCache:
    """What incremental decoding keeps between steps, owned by the caller (BaseDecoder.empty_cache, make_cache):
    self_k / self_v  per layer (B, H, max_len, hd): the self-attention keys / values of positions decoded so far;
    memory_kv        per layer (B, S, 2, H, hd): the cross-attention projection of the encoder memory;
    memory_mask      (B, S) uint8 source key-padding mask (non-zero = PAD) or None;
    pad              (B, max_len) uint8: pad[:, j] != 0 where target token j is PAD. The caller sets column t before
                     step t (column 0, BOS, is 0); it is the key-padding half of make_std_mask, the causal half
                     being the cache length itself.
    head_pad         None, or (B, H, max_len) uint8: the per-head key mask of the reference's decode()
                     (base_seq2seq.py:99-114). It hands nn.MultiheadAttention `tgt_mask.repeat(num_heads, 1, 1)`,
                     which that module reads as (B, H, T, T): head h of sample b sees the PAD columns of sample
                     (b * H + h) % B. BaseDecoder.step copies column t of pad into this layout before step t.
    Beam search (make_cache(..., beam=W)): self_k / self_v and pad hold R = B * W hypothesis rows while memory_kv and
    memory_mask keep B rows, shared by the kv_group = W rows of an AST, and
    anc              (R, max_len) int32: anc[r, j] = the self_k / self_v row that holds key j of hypothesis r. A
                     hypothesis' history stays where its ancestors stored it; beam_select rewrites this table, never
                     the cache."""

    def __init__(self, self_k, self_v, memory_kv, memory_mask, pad, head_pad=None, anc=None, kv_group=1):
        self.self_k, self.self_v, self.memory_kv = self_k, self_v, memory_kv
        self.memory_mask, self.pad, self.head_pad = memory_mask, pad, head_pad
        self.anc, self.kv_group = anc, kv_group

    @property
    def self_mask(self):
        return self.pad if self.head_pad is None else self.head_pad


class BaseDecoder(nn.Module):
    def __init__(self, decoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = _clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.norm = norm

    def forward(self, tgt, memory, tgt_mask, memory_key_padding_mask=None):
        out, w = tgt, None
        for mod in self.layers:
            out, w = mod(out, memory, tgt_mask=tgt_mask, memory_key_padding_mask=memory_key_padding_mask)
        return (self.norm(out) if self.norm is not None else out), w

    def forward_fused(self, tgt, memory, tgt_pad=None, memory_key_padding_mask=None, mask_mode="own", kv_group=1):
        """forward() for batch-first tgt (R, T, E) and an UN-repeated batch-first memory (B, S, E), R = B * kv_group,
        on the fused full-sequence attention (DecoderLayer.forward_fused): tgt_pad (R, T) uint8 / bool replaces the
        (R * H, T, T) float mask (mask_mode "own": forward()'s mask.repeat_interleave(H, 0); "reference": its
        mask.repeat(H, 1, 1)), memory_key_padding_mask is the (B, S) mask. Returns (R, T, E). self.last_fused: every
        attention of the call ran seq_attention (False: a module in training mode with dropout > 0 took SDPA)."""
        out = tgt
        for mod in self.layers:
            out = mod.forward_fused(out, memory, tgt_pad, memory_key_padding_mask, mask_mode, kv_group)
        self.last_fused = all(a.last_fused for mod in self.layers for a in (mod.self_attn, mod.multihead_attn))
        return self.norm(out) if self.norm is not None else out

    def empty_cache(self, B, max_len, device, dtype, repeat_heads=False, beam=None, S=None, group=None):
        """A zeroed DecodeCache for B memory rows and up to max_len target positions: the one place that spells the
        layout (see DecodeCache). repeat_heads: key-pad the heads as forward() does when given
        make_std_mask(...).repeat(num_heads, 1, 1), the reference's decode(); otherwise head h of sample b sees sample
        b's PAD columns (a (B*H, T, T) mask built by repeat_interleave). beam=W: the cache of a beam search of width W,
        R = B * W self-attention rows, pad rows and ancestry rows over the B memory rows and the (B, S) memory mask (not
        with repeat_heads). S: also static memory_kv / memory_mask buffers for S source keys, which load_memory fills
        in place (a captured graph keeps reading them); without S the memory side is left to the caller.
        group=G: a group without ancestry, R = B * G self-attention and pad rows that each keep their own cache row
        (anc stays None) over the B memory rows, kv_group = G: the independent samples of SamplingGenerator (not with
        beam or repeat_heads)."""
        attn = self.layers[0].self_attn
        H, hd = attn.num_heads, attn.embed_dim // attn.num_heads
        if beam is not None and (repeat_heads or beam < 1):
            raise ValueError("make_cache: beam is a positive width and does not go with repeat_heads")
        if group is not None and (repeat_heads or beam is not None or group < 1):
            raise ValueError("make_cache: group is a positive count and does not go with beam or repeat_heads")
        R = B if beam is None else B * beam
        if group is not None:
            R = B * group
        z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=device)
        kv = [z(2, R, H, max_len, hd) for _ in self.layers]
        return DecodeCache(self_k=[c[0] for c in kv], self_v=[c[1] for c in kv],
                           memory_kv=None if S is None else [z(B, S, 2, H, hd) for _ in self.layers],
                           memory_mask=None if S is None else z(B, S, dt=torch.uint8),
                           pad=z(R, max_len, dt=torch.uint8),
                           head_pad=z(B, H, max_len, dt=torch.uint8) if repeat_heads else None,
                           anc=None if beam is None else z(R, max_len, dt=torch.int32),
                           kv_group=group if group is not None else 1 if beam is None else beam)

    def load_memory(self, cache, memory, memory_key_padding_mask):
        """A new batch-first memory (B, S, E) into the static buffers of an empty_cache(..., S=S) cache: every layer's
        cross-attention projection and the key-padding mask (None: no key is masked, the buffer is zeroed)."""
        for kv, mod in zip(cache.memory_kv, self.layers):
            kv.copy_(mod.multihead_attn.project_memory(memory))
        if memory_key_padding_mask is None:
            cache.memory_mask.zero_()
        else:
            cache.memory_mask.copy_(memory_key_padding_mask)

    def make_cache(self, memory, memory_key_padding_mask, max_len, repeat_heads=False, beam=None, group=None):
        """empty_cache for a batch-first memory (B, S, E), holding the memory projections themselves (no copy) and the
        mask as uint8, or None without one."""
        cache = self.empty_cache(memory.shape[0], max_len, memory.device, memory.dtype, repeat_heads, beam, group=group)
        cache.memory_kv = [mod.multihead_attn.project_memory(memory) for mod in self.layers]
        if memory_key_padding_mask is not None:
            cache.memory_mask = memory_key_padding_mask.to(torch.uint8).contiguous()
        return cache

    def step(self, x, cache, t):
        """forward() in eval mode for the single target position t: x (B, 1, E) batch-first -> (B, 1, E), equal to
        row t of forward() over positions 0..t (the decoder is causal and cache.pad carries the PAD keys).
        t is an int, or the device counter (1-element int32 tensor) of device-stepped decoding: the attention kernels
        then read the step themselves, and column t of head_pad has been written by the previous step's
        argmax_rows(..., t_dev=, head_pad=), so nothing is copied here."""
        if cache.head_pad is not None and not isinstance(t, torch.Tensor):  # rows r = h' * B + b' of the (B*H) layout hold pad[b'] (mask.repeat(H, 1, 1))
            B, H, _ = cache.head_pad.shape
            cache.head_pad.view(H, B, -1)[:, :, t] = cache.pad[:, t]
        for i, mod in enumerate(self.layers):
            x = mod.step(x, cache, i, t)
        return self.norm(x) if self.norm is not None else x


class Generator(nn.Module):
    """components.py:95-102 Generator: log(softmax(dropout(linear(x))))  (log of softmax, not
    log_softmax). The linear stays on hipBLASLt; dropout + softmax + log is one HIP kernel per
    direction (csa_amd/gen_ops.py, csrc/csa_gen.hip). Module/param names as the reference."""

    def __init__(self, tgt_vocab_size, hidden_size, dropout):
        super().__init__()
        self.soft_max = nn.Softmax(-1)
        self.dropout = nn.Dropout(dropout)
        self.linear = Linear(hidden_size, tgt_vocab_size)

    def forward(self, x):
        from .gen_ops import gen_log_softmax
        return gen_log_softmax(self.linear(x), self.dropout.p if self.training else 0.0)


def make_std_mask(tgt, pad=PAD):
    """dataset/base_data_set.py:125-135: pad | future mask, (B,T,T) bool."""
    T = tgt.size(-1)
    future = torch.triu(torch.ones(T, T, dtype=torch.bool, device=tgt.device), diagonal=1)
    return (tgt == pad).unsqueeze(-2) | future.unsqueeze(0)


class TreePositionalEncodings(nn.Module):
    """module/csa_trans.py:19-64 (Shiv & Quirk 2019): positions (bs, n, depth * degree) -> (bs, n, depth * degree *
    n_feat), weighted by tanh(p)^level * sqrt((1 - tanh(p)^2) d_model / 2). The reference's name, constructor and
    parameter `p`; on the GPU one HIP kernel per direction (pe_ops.tree_pos_encode)."""

    def __init__(self, depth, degree, n_feat, d_model):
        super().__init__()
        self.depth = depth
        self.width = degree
        self.d_pos = n_feat * depth * degree
        self.d_model = d_model
        self.d_tree_param = self.d_pos // (self.depth * self.width)
        self.p = nn.Parameter(torch.ones(self.d_tree_param, dtype=torch.float32), requires_grad=True)
        self.init_weights()

    def init_weights(self):
        self.p.data.uniform_(0.7, 0.999)

    def build_weights(self):
        from .pe_ops import tree_weights
        return tree_weights(self.p, self.depth, self.width, self.d_model)

    def forward(self, positions):
        from .pe_ops import tree_pos_encode
        return tree_pos_encode(positions, self.p, self.depth, self.width, self.d_model)


USE_PEGEN = ("pegen", "laplacian", "sequential", "treepos", "triplet")


class CSATrans(nn.Module):
    """module/csa_trans.py:67-177 (+ BaseTrans.forward/encode/decode, base_seq2seq.py:40-114). use_pegen picks the
    structure encoding fed to the SBM encoder: "pegen" (the CSE layers), or one of the paper's ablations, "laplacian"
    (data.lap_pe, or the device eigenvectors of data.adj), "sequential" (sinusoidal, inside SBM), "treepos"
    (data.tree_pos) and "triplet" (data.triplet); each has the reference's parameters and state_dict keys.
    triplet_vocab_size is the size of the triplet embedding (the reference's 1246; its commented-out java value
    is 1505)."""

    def __init__(self, src_vocab_size, tgt_vocab_size, hidden_size, num_heads, num_layers, sbm_layers, use_pegen,
                 dim_feed_forward, dropout, pe_dim, pegen_dim, sbm_enc_dim, clusters, full_att, state_dict=None,
                 max_src_len=150, return_maps=False, triplet_vocab_size=1246):
        super().__init__()
        if use_pegen not in USE_PEGEN:
            raise ValueError(f"use_pegen must be one of {USE_PEGEN}")
        self.num_heads = num_heads
        self.pe_dim, self.pegen_dim = pe_dim, pegen_dim
        self.use_pegen = use_pegen
        self.src_embedding = Embeddings(sbm_enc_dim - pe_dim, src_vocab_size, dropout, with_pos=False)
        self.tgt_embedding = Embeddings(hidden_size, tgt_vocab_size, dropout, with_pos=True)
        if use_pegen == "pegen":
            self.src_pe_embedding = Embeddings(pegen_dim, src_vocab_size, dropout, with_pos=False)
            self.pegen = CSE(CSE_layer(pegen_dim, num_heads, pegen_dim, dropout), num_layers, num_heads, pegen_dim,
                             dropout=dropout, max_src_len=max_src_len)
        elif use_pegen == "treepos":
            self.tree_pos_enc = TreePositionalEncodings(depth=16, degree=8, n_feat=pegen_dim // 128, d_model=pegen_dim)
        elif use_pegen == "triplet":
            self.triplet_emb = nn.Embedding(triplet_vocab_size, pegen_dim)
        config = {"sbm_layers": sbm_layers, "transformer_dim": sbm_enc_dim, "transformer_hidden_dim": sbm_enc_dim,
                  "head_dim": sbm_enc_dim // num_heads, "num_head": num_heads, "attn_type": "sbm",
                  "attention_grad_checkpointing": False, "attention_dropout": 0.2, "num_clusters": clusters,
                  "dropout_prob": 0.2, "out_dim": hidden_size, "max_src_len": max_src_len, "full_att": full_att,
                  "return_maps": return_maps}
        self.SBM = SBM(config, sbm_enc_dim, pe_dim, pegen_dim, use_pegen)
        self.decoder = BaseDecoder(DecoderLayer(hidden_size, num_heads, dim_feed_forward, dropout, "gelu"), 4,
                                   norm=LayerNorm(hidden_size))
        self.generator = Generator(tgt_vocab_size, hidden_size, dropout)
        if state_dict is None:
            for p in self.parameters():
                if p.dim() > 1:
                    nn.init.xavier_uniform_(p)
            if not full_att:
                for i in range(sbm_layers):
                    nn.init.orthogonal_(getattr(self.SBM, f"transformer_{i}").mha.attn.layer.weight)
        else:
            self.load_state_dict(state_dict)

    def base_process(self, data):
        """base_seq2seq.py:43-54: masks and embeddings; the target side only when tgt_seq is given
        (GreedyGenerator runs with tgt_seq None and fills tgt_mask / tgt_emb per step)."""
        data.src_mask = data.src_seq.eq(PAD)
        data.src_emb = self.src_embedding(data.src_seq)
        if self.use_pegen == "pegen":
            data.src_pe_emb = self.src_pe_embedding(data.src_seq)
        if getattr(data, "tgt_seq", None) is not None:
            data.tgt_mask = make_std_mask(data.tgt_seq, PAD)
            data.tgt_emb = self.tgt_embedding(data.tgt_seq)

    def process_data(self, data):
        """base_seq2seq.py:56-57. A batch that carries data.parents and data.num_node but no data.L (data.collate_parents,
        synthetic_batch(planes=False)) gets what this model's use_pegen reads, and nothing more, built on its device by
        batch_ops.ast_batch: rel / rel_mask (and their L, T, L_mask, T_mask views), adj, tree_pos or triplet. A field
        the batch already carries is kept."""
        if getattr(data, "L", None) is None and getattr(data, "parents", None) is not None:
            from .batch_ops import FIELDS_OF_MODE, ast_batch
            need = tuple(f for f in FIELDS_OF_MODE[self.use_pegen] if getattr(data, f, None) is None)
            if self.use_pegen == "laplacian" and getattr(data, "lap_pe", None) is not None:
                need = ()  # encode takes the precomputed eigenvectors
            if need:
                built = vars(ast_batch(data.parents, data.num_node, fields=need))
                for f in need + tuple(k for k in ("rel", "rel_mask") if k in built):
                    setattr(data, f, built[f])
        self.base_process(data)

    def encode(self, data):
        """base_seq2seq.py:67-97: the structure encoding -> SBM; sparsity = mean over the SBM layers' head
        sparsities, or 1 for the dense ablation. Returns (enc, sparsity, pe, graphs, attns). The laplacian mode takes
        data.lap_pe, a precomputed (B, N, pegen_dim) tensor (what a dataset would cache), when the batch carries one,
        and otherwise computes the eigenvectors of data.adj on the device (pe_ops.lap_pe) instead of the reference's
        per-AST host eigh."""
        mode = self.use_pegen
        if mode == "pegen":
            src_pe = self.pegen(data)
        elif mode == "laplacian":
            src_pe = getattr(data, "lap_pe", None)
            if src_pe is None:
                from .pe_ops import lap_pe
                src_pe = lap_pe(data.adj, data.num_node, self.pegen_dim).pe
        elif mode == "treepos":
            src_pe = self.tree_pos_enc(data.tree_pos)
        elif mode == "triplet":
            src_pe = self.triplet_emb(data.triplet)
        else:  # sequential: SBM adds its own sinusoidal encoding
            src_pe = None
        enc, sparsity, graphs, attns, pe = self.SBM(data, src_pe, self.use_pegen)
        sparsity = 1 if sparsity[0] is None else torch.mean(torch.stack(sparsity))
        return enc, sparsity, pe, graphs, attns

    def decode(self, data, encoder_outputs):
        """base_seq2seq.py:99-114: returns (decoder outputs (B,T,E), last cross-attention weights)."""
        tgt_mask = data.tgt_mask.repeat(self.num_heads, 1, 1)
        dec, w = self.decoder(data.tgt_emb.permute(1, 0, 2), encoder_outputs.permute(1, 0, 2), tgt_mask=tgt_mask,
                              memory_key_padding_mask=data.src_mask)
        return dec.permute(1, 0, 2), w

    def forward(self, data):
        """base_seq2seq.py:59-65."""
        self.process_data(data)
        enc, sparsity, pe, graphs, attns = self.encode(data)
        dec, _ = self.decode(data, enc)
        out = self.generator(dec)
        return out, sparsity, pe, graphs, attns


class GreedyGenerator(nn.Module):
    """module/base_seq2seq.py:117-145: one encode, then max_tgt_len-1 steps of decode + generator +
    argmax over the last position, starting from BOS; returns the generated ids without BOS."""

    def __init__(self, model, max_tgt_len, multi_gpu=False):
        super().__init__()
        self.model = model.module if multi_gpu else model
        self.max_tgt_len = max_tgt_len
        self.start_pos = BOS
        self.unk_pos = UNK

    def forward(self, data):
        m = self.model
        m.process_data(data)
        enc, _, _, _, _ = m.encode(data)
        ys = torch.full((enc.size(0), 1), self.start_pos, dtype=torch.long, device=enc.device)
        for _ in range(self.max_tgt_len - 1):
            data.tgt_mask = make_std_mask(ys, PAD)
            data.tgt_emb = m.tgt_embedding(ys)
            dec, _ = m.decode(data, enc)
            out = m.generator(dec)[:, -1, :]
            next_word = torch.max(out, dim=1)[1]
            ys = torch.cat([ys, next_word.unsqueeze(1)], dim=1)
        return ys[:, 1:]


_DECODING = ("DecodingConstraints", "_SteppedDecoding", "CachedGreedyGenerator", "BeamSearchGenerator",
             "SamplingGenerator")
_SCORING = ("SequenceScorer", "rerank", "validation_nll", "ATTENTIONS")
_SEQ_ATTN = ("seq_attention",)


def __getattr__(name):
    """The names of csa_amd.decoding, exported from here as before they moved. That module imports this one
    (CachedGreedyGenerator subclasses GreedyGenerator), so it is imported on first use, not while this one loads.
    The names of csa_amd.scoring (scoring given summaries under the model) are exported the same way."""
    if name in _DECODING:
        from . import decoding
        return getattr(decoding, name)
    if name in _SCORING:
        from . import scoring
        return getattr(scoring, name)
    if name in _SEQ_ATTN:  # the fused full-sequence decoder attention behind SequenceScorer(attention="fused")
        from . import seq_attn_ops
        return getattr(seq_attn_ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class _GatherTargets(torch.autograd.Function):
    """x.gather(1, t[:, None])[:, 0] whose backward scatters into a fresh zero tensor in place (torch's
    gather backward is an out-of-place scatter_add, i.e. zeros + a full clone of the (B*T, V) grad)."""

    @staticmethod
    def forward(ctx, x, t):
        ctx.save_for_backward(t)
        ctx.shape = x.shape
        return x.gather(1, t.unsqueeze(1)).squeeze(1)

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        gx = torch.zeros(ctx.shape, device=g.device, dtype=g.dtype)
        gx.scatter_add_(1, t.unsqueeze(1), g.unsqueeze(1))
        return gx, None


def _gather_targets(x, t):
    return _GatherTargets.apply(x, t)


class LabelSmoothing(nn.Module):
    """utils/label_smooth.py:15-40 without materialising true_dist (B*T x V: 251 MB per step at the java
    config). true_dist is `confidence` at the target, 0 in the padding column and in padded rows, and
    eps = smoothing / (V - 2) elsewhere, so the KLDiv(sum) / ntokens closes to, per non-pad row,
        conf (log conf - x_t) + eps ((V-2) log eps - sum_{j != t, pad} x_j)
    (the row sum is read only when smoothing > 0). torch's kl_div gives 0 * (-inf) = NaN wherever
    true_dist is 0 and x is -inf (an underflowed log-probability); that NaN is reproduced with one
    detached compare over x. ntokens = (target != 0).sum() literally, as the reference."""

    def __init__(self, padding_idx, smoothing=0.0):
        super().__init__()
        self.padding_idx = padding_idx
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        self.true_dist = None  # never materialised

    def forward(self, x, target):
        V = x.size(-1)
        x = x.reshape(-1, V)
        t = target.reshape(-1)
        ntokens = (target != 0).sum()
        valid = t != self.padding_idx
        xt = _gather_targets(x, t)
        conf, sm = self.confidence, self.smoothing
        row = -conf * xt + (conf * math.log(conf) if conf > 0.0 else 0.0)
        with torch.no_grad():
            if sm > 0.0:
                bad = ~(x > float("-inf"))  # -inf or NaN
                n_bad = bad.sum()
                n_at_td = (bad[valid].sum() - bad[valid, self.padding_idx].sum()) if V > 2 else 0
            else:
                # per-row fp32 counts (exact: V < 2^24) summed in fp64: a bool .sum() would first cast
                # the whole (B*T, V) mask to int64 (500 MB at the java config)
                n_bad = torch.where(x > float("-inf"), 0.0, 1.0).sum(1).double().sum()
                n_at_td = (~(xt.detach() > float("-inf")) & valid).sum()
            poison = torch.where(n_bad > n_at_td, float("nan"), 0.0).to(x.dtype)
        if sm > 0.0:
            eps = sm / (V - 2)
            col = torch.arange(V, device=x.device).unsqueeze(0)
            off = (col == t.unsqueeze(1)) | (col == self.padding_idx)  # true_dist != eps there
            rest = torch.where(off, torch.zeros_like(x), x).sum(1)
            row = row + eps * ((V - 2) * math.log(eps) - rest)
        loss = torch.where(valid, row, torch.zeros_like(row)).sum() + poison
        return loss / ntokens


def label_smoothing_loss(logp, target, padding_idx=PAD):
    """LabelSmoothing(padding_idx, smoothing=0) as a function (all configs use smoothing 0)."""
    return LabelSmoothing(padding_idx, 0.0)(logp, target)


def batch_to_device(sb, device):
    """Synthetic batch dict (csa_amd.data.synthetic_batch) -> device-resident namespace."""
    g = lambda k, dt=None: torch.as_tensor(sb[k], dtype=dt).to(device, non_blocking=True)
    if "L" not in sb:  # synthetic_batch(planes=False): the parent arrays; process_data builds the fields on the device
        data = SimpleNamespace(src_seq=g("src_seq", torch.int64), tgt_seq=g("tgt_seq", torch.int64),
                               parents=g("parents", torch.int32), num_node=g("num_node", torch.int32))
        if "lap_pe" in sb:
            data.lap_pe = g("lap_pe", torch.float32)
        return data, g("target", torch.int64)
    data = SimpleNamespace(src_seq=g("src_seq", torch.int64), tgt_seq=g("tgt_seq", torch.int64),
                           L=g("L", torch.uint8), T=g("T", torch.uint8), L_mask=g("L_mask", torch.uint8),
                           T_mask=g("T_mask", torch.uint8))
    # the ablation fields (synthetic_batch(..., ablation_fields=True)), and a precomputed lap_pe, when present
    for k, dt in (("adj", torch.uint8), ("tree_pos", torch.float32), ("triplet", torch.int64),
                  ("num_node", torch.int32), ("lap_pe", torch.float32)):
        if k in sb and (k != "num_node" or "adj" in sb):
            setattr(data, k, g(k, dt))
    return data, g("target", torch.int64)


CONFIGS = {  # config/python.py, config/java.py, config/python_full_att.py (vocab sizes: create_vocab caps)
    "python": dict(src_vocab_size=10000, tgt_vocab_size=20000, hidden_size=512, num_heads=8, num_layers=4,
                   sbm_layers=4, use_pegen="pegen", dim_feed_forward=2048, dropout=0.2, pe_dim=256,
                   pegen_dim=512, sbm_enc_dim=512, clusters=[10, 10, 10, 10], full_att=False),
    "java": dict(src_vocab_size=10000, tgt_vocab_size=20000, hidden_size=512, num_heads=8, num_layers=4,
                 sbm_layers=4, use_pegen="pegen", dim_feed_forward=2048, dropout=0.2, pe_dim=128, pegen_dim=512,
                 sbm_enc_dim=768, clusters=[10, 10, 10, 10], full_att=False),
    "python_full_att": dict(src_vocab_size=10000, tgt_vocab_size=20000, hidden_size=512, num_heads=8,
                            num_layers=4, sbm_layers=4, use_pegen="pegen", dim_feed_forward=2048, dropout=0.2,
                            pe_dim=256, pegen_dim=512, sbm_enc_dim=512, clusters=[10, 10, 10, 10], full_att=True),
}
