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
"""
import copy
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .data import BOS, EOS, UNK
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
        rel = torch.stack([data.L, data.T], 1)          # (B,2,N,N) uint8: heads 0-3 read L, 4-7 read T
        mask = torch.stack([data.L_mask, data.T_mask], 1)
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
        """base_seq2seq.py:56-57."""
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


@dataclass(frozen=True)
class DecodingConstraints:
    """Which tokens a decoding step may choose, for CachedGreedyGenerator, BeamSearchGenerator and SamplingGenerator
    (decode_ops.constrain_rows, csrc/csa_constrain.hip): a frozen, hashable value.

    repetition_penalty theta > 0 (1: off): the logit z of every token already in the row's history, BOS included,
    becomes z / theta if z > 0 else z * theta, once however often the token occurs. no_repeat_ngram_size n >= 0 (0: off):
    a token that would complete an n-gram the history already holds is banned. min_length: eos_id is banned at the
    steps t < min_length, so an output holds at least min_length tokens before its EOS (off at 0 or with eos_id None).
    suppress_ids: at most 256 ids banned at every step. A banned token is a -inf logit to the selection that follows,
    which renormalises over what is left. `active` is False when every rule is off; the generators then run exactly
    the launches they run without constraints."""

    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_length: int = 0
    suppress_ids: tuple = ()
    eos_id: Optional[int] = EOS

    MAX_SUPPRESS = 256

    def __post_init__(self):
        theta = float(self.repetition_penalty)
        if not 0.0 < theta < float("inf"):
            raise ValueError("DecodingConstraints: repetition_penalty must be positive and finite (1 turns it off)")
        for name in ("no_repeat_ngram_size", "min_length"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < 0:
                raise ValueError(f"DecodingConstraints: {name} must be a non-negative integer (0 turns it off)")
        ids, eos = tuple(self.suppress_ids), self.eos_id
        if len(ids) > self.MAX_SUPPRESS or any(isinstance(i, bool) or int(i) != i or not 0 <= i < 2 ** 31 for i in ids):
            raise ValueError("DecodingConstraints: suppress_ids holds at most 256 non-negative integer ids")
        if eos is not None and (isinstance(eos, bool) or int(eos) != eos or eos < 0):
            raise ValueError("DecodingConstraints: eos_id must be a non-negative integer or None")
        for name, v in (("repetition_penalty", theta), ("no_repeat_ngram_size", int(self.no_repeat_ngram_size)),
                        ("min_length", int(self.min_length)), ("suppress_ids", tuple(int(i) for i in ids)),
                        ("eos_id", None if eos is None else int(eos))):
            object.__setattr__(self, name, v)  # the normalised value (frozen: no plain assignment)

    @property
    def active(self):
        return (self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or bool(self.suppress_ids)
                or (self.min_length > 0 and self.eos_id is not None))

    def apply(self, logits, ys, t, fin=None, suppress=None):
        """One constrain_rows call with this value's rules; suppress: suppress_tensor(device) made once."""
        from .decode_ops import constrain_rows
        return constrain_rows(logits, ys, t, fin=fin, repetition_penalty=self.repetition_penalty,
                              no_repeat_ngram=self.no_repeat_ngram_size, min_length=self.min_length, eos_id=self.eos_id,
                              suppress=suppress)

    def suppress_tensor(self, device):
        """The suppress list as the static int32 device tensor that the kernel reads, or None for an empty list."""
        return torch.tensor(self.suppress_ids, dtype=torch.int32, device=device) if self.suppress_ids else None


class _SteppedDecoding:
    """graph=True of CachedGreedyGenerator and BeamSearchGenerator: the device-stepped decode step (every kernel reads
    the step from the 4-byte device counter e.t_dev, so every step issues the same launches), captured once per
    (device, B, S, max_tgt_len, the generator's key extras, parameter addresses) as one single-stream
    torch.cuda.CUDAGraph over static buffers and replayed max_tgt_len - 1 times per call. `captures` counts the graphs
    captured. The generator supplies _state(cache, **kw), _reset(e), _device_step(e) and, if it must, _check_capture.

    constraints= (a DecodingConstraints) is shared by the three generators: when active, one decode_ops.constrain_rows
    call sits between generator.linear and the selection of every step, the value joins the graph key extras and the
    suppress list is a static device tensor of the state; None or an inactive value changes nothing.

    early_stop=True (needs an eos_id, so a finished flag e.fin per row) is one rule for the three generators: decoding
    stops after the first step that BEGAN with every row finished, one step after the step s that finished the last
    row, so steps 0..s+1 run; without such a step all max_tgt_len - 1 run. The extra step is the one after which the
    state is a fixed point (for the beam, the step in which the selection orders the all-finished hypotheses by cum), so
    ids, scores and log-probabilities are bitwise those of the full run; columns never written stay PAD / 0 as _reset
    leaves them. On the device the rule is a latch: the step ends with decode_ops.decode_advance in place of the
    counter's increment, which counts the step in the state words e.stop = {all_prev, steps_run, parked, 0} and parks
    the counter at -1; every step kernel returns on a negative counter, so a surplus replay stores nothing. The host
    (_run_steps) issues replays in chunks of poll_every, copies the state words to a pinned buffer after each chunk
    (outside the graph, same stream, non-blocking) and, before issuing chunk k + 2, waits for chunk k's copy and stops
    if it reports parked: at most two chunks are ever in flight and no kernel waits on the host. last_steps_run is the
    latch's count after the call (max_tgt_len - 1 without early_stop), exact whatever the chunking; last_replays is
    the number of steps issued, at most last_steps_run + 2 * poll_every. False keeps the launches, the graph key and
    the captured graph of a generator built without the keyword."""

    MAX_GRAPHS = 4  # captured (shape, weights) entries kept per generator; the oldest is evicted
    POLL_EVERY = 2  # replays per chunk of an early-stopping graph=True call: the fastest of 2, 4 and 8
                    # (tools/bench_early_stop.py, profiles/early_stop_decode.json)

    def _init_stepped(self, graph, early_stop=False, **cache_options):
        self.graph = graph
        self.captures = 0      # graphs captured so far (graph=True on a CUDA model; 0 otherwise)
        self._graphs = {}      # key -> SimpleNamespace of static buffers and the captured step (insertion-ordered)
        self._keep_graph = False  # keep the captured hipGraph_t (tools/bench_greedy.py counts its nodes)
        self._cache_options = cache_options  # what the generator asks of BaseDecoder.empty_cache
        self.early_stop = bool(early_stop)
        self.poll_every = self.POLL_EVERY
        self.last_steps_run = None  # decode steps that ran in the last call
        self.last_replays = None    # decode steps issued in the last call (>= last_steps_run: parked ones store nothing)
        self._check_early_stop()

    def _check_early_stop(self):
        if self.early_stop and self.eos_id is None:
            raise ValueError(f"{type(self).__name__}: early_stop=True needs an eos_id (without one no row ever finishes)")

    def _stop_key(self):
        """What early_stop adds to the graph key extras: nothing when it is off."""
        return ("early_stop",) if self.early_stop else ()

    def _stop_state(self, device):
        """The latch's state words {all_prev, steps_run, parked, reserved} of a step's state (None without early_stop)."""
        return torch.zeros(4, dtype=torch.int32, device=device) if self.early_stop else None

    def _advance(self, e):
        """The end of a device step, after the counter's last reader: the increment, or the early-stop latch."""
        if e.stop is None:
            e.t_dev.add_(1)
        else:
            from .decode_ops import decode_advance
            decode_advance(e.fin, e.t_dev, e.stop, self.max_tgt_len)

    def _run_steps(self, e, graphed, after_step=None):
        """The decode steps of one call on the reset state e: replays of e.graph (graphed) or eager _device_step calls,
        max_tgt_len - 1 of them or, with early_stop, until the latch reports parked (see the class docstring).
        after_step() runs on the host after each issued step. Sets last_steps_run and last_replays."""
        self._check_early_stop()
        n = self.max_tgt_len - 1
        step = e.graph.replay if graphed else (lambda: self._device_step(e))
        if e.stop is None:
            for _ in range(n):
                step()
                if after_step is not None:
                    after_step()
            self.last_steps_run = self.last_replays = n
            return
        issued = 0
        if not graphed:  # host-bound already: read the latch after every step
            while issued < n:
                step()
                issued += 1
                if after_step is not None:
                    after_step()
                if int(e.stop[2]) != 0:
                    break
            self.last_steps_run, self.last_replays = int(e.stop[1]), issued
            return
        poll = max(1, int(self.poll_every))
        chunks = (n + poll - 1) // poll
        if e.stop_host is None or e.stop_host.shape[0] < chunks + 1:
            e.stop_host = torch.empty(chunks + 1, 4, dtype=torch.int32, pin_memory=True)
        stream = torch.cuda.current_stream(e.stop.device)
        events = []
        while issued < n:
            k = len(events)
            if k >= 2:  # chunks k - 1 and k - 2 are in flight: wait for the older one's state words
                events[k - 2].synchronize()
                if int(e.stop_host[k - 2, 2]) != 0:
                    break
            for _ in range(min(poll, n - issued)):
                step()
                issued += 1
                if after_step is not None:
                    after_step()
            e.stop_host[k].copy_(e.stop, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            events.append(ev)
        e.stop_host[chunks].copy_(e.stop, non_blocking=True)
        stream.synchronize()
        self.last_steps_run, self.last_replays = int(e.stop_host[chunks, 1]), issued

    @property
    def constraints(self):
        """The active DecodingConstraints, or None. Assignable between calls: None and an inactive value are the same
        thing, no constraint step at all (the launches, the graph key and the captured graph of a generator built
        without the keyword); another active value gets a captured graph of its own."""
        return self._constraints

    @constraints.setter
    def constraints(self, constraints):
        if constraints is not None and not isinstance(constraints, DecodingConstraints):
            raise TypeError("constraints must be a DecodingConstraints or None")
        object.__setattr__(self, "_constraints", constraints if constraints is not None and constraints.active else None)

    def _suppress_state(self, device):
        """The suppress list as the static device tensor of a step's state (None without one)."""
        return None if self.constraints is None else self.constraints.suppress_tensor(device)

    def _constraint_key(self):
        """What the constraints add to the graph key extras: nothing when there are none."""
        return () if self.constraints is None else (self.constraints,)

    def _check_constraints_capture(self, enc):
        from ._lib import lib
        if self.constraints is not None and (not lib().csa_constrain_rows_supported(self.max_tgt_len)
                                             or enc.dtype != torch.float32):
            raise ValueError(f"{type(self).__name__}: graph=True with constraints needs fp32 and max_tgt_len <= 1024 "
                             "(csa_constrain_rows_supported)")

    def _step_params(self):
        m = self.model
        mods = (m.tgt_embedding, m.decoder, m.generator.linear)
        return [p for mod in mods for p in list(mod.parameters()) + list(mod.buffers())]

    def _check_capture(self, enc):
        """Raises where the generator's step cannot be captured for this memory."""
        self._check_constraints_capture(enc)

    def _capture(self, enc, **state_kw):
        self._check_capture(enc)
        dev = enc.device
        cache = self.model.decoder.empty_cache(enc.size(0), self.max_tgt_len, dev, enc.dtype, S=enc.size(1),
                                               **self._cache_options)
        e = self._state(cache, **state_kw)
        self._reset(e)
        # one eager device-stepped step on a side stream first: code objects, hipBLASLt heuristics and workspaces
        # are then in place and stay outside the capture
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._device_step(e)
        torch.cuda.current_stream(dev).wait_stream(side)
        e.graph = torch.cuda.CUDAGraph(keep_graph=True) if self._keep_graph else torch.cuda.CUDAGraph()
        with torch.cuda.graph(e.graph):  # a single capture stream: the captured step has no parallel branches
            self._device_step(e)
        if self._keep_graph:
            e.graph.instantiate()
        self.captures += 1
        return e

    def _graph_entry(self, enc, src_mask, key_extra, **state_kw):
        """The captured entry for this memory (captured now if there is none, the oldest evicted), its static memory
        buffers loaded from enc and src_mask and its state reset to step 0: ready for max_tgt_len - 1 replays."""
        B, S, T = enc.size(0), enc.size(1), self.max_tgt_len
        # reallocated parameters recapture; weights updated in place are simply read by the next replay
        key = (enc.device, B, S, T, *key_extra, tuple(p.data_ptr() for p in self._step_params()))
        e = self._graphs.get(key)
        if e is None:
            with torch.cuda.device(enc.device):
                e = self._capture(enc, **state_kw)
            while len(self._graphs) >= self.MAX_GRAPHS:
                del self._graphs[next(iter(self._graphs))]
            self._graphs[key] = e
        self.model.decoder.load_memory(e.cache, enc, src_mask)
        self._reset(e)
        return e


class CachedGreedyGenerator(_SteppedDecoding, GreedyGenerator):
    """GreedyGenerator with a key/value cache: the same tokens from one decoder pass per NEW position.

    The decoder is causal and the key-padding mask of positions <= j never changes as ys grows, so step t needs only
    position t: its embedding, BaseDecoder.step against the cached self-attention keys / values and the once-projected
    encoder memory (csa_decode_attn), the Generator's linear on the B last rows, and the row argmax written into
    ys[:, t+1] with the next step's PAD byte (csa_argmax_rows). Eval-mode log(softmax(z)) is monotone in z, so the
    argmax of the logits is the reference's torch.max(out, 1)[1] and the softmax is skipped unless return_logp asks for
    the (max_tgt_len-1, B, V) last-position log-probabilities. All max_tgt_len-1 steps run, as in the reference, unless
    early_stop asks otherwise (below). In training mode this defers to GreedyGenerator.

    graph=True (eval mode, CUDA model): the loop above is bound by the host, about 70 small launches per step issued
    from Python. The step is instead run device-stepped (csa_decode_embed, csa_decode_attn_step, csa_argmax_rows_step)
    and replayed from one captured graph per (..., return_logp, ...) (_SteppedDecoding); process_data, encode (its
    Philox key comes from the CPU generator) and the memory projections stay eager. Same ids and log-probabilities,
    bitwise.

    constraints=DecodingConstraints(...): the logits of every step go through decode_ops.constrain_rows before the
    argmax (history = the row's tokens so far, BOS included; there is no finished flag here, so the rules keep applying
    after an EOS), and return_logp reports the constrained distribution. Training mode with active constraints
    raises: the uncached loop it defers to has no such step.

    eos_id (default None: the behaviour above, bit for bit): the generator keeps a finished flag per row, fin (B,) uint8.
    A row that has emitted eos_id takes PAD from then on (csa_argmax_rows_fin_step) and active constraints leave it
    alone. With the head-repeated PAD mask a finished row's PAD columns enter other rows' masks, so this is a behaviour
    of its own, not a truncation of the ids without eos_id. early_stop=True (needs eos_id; _SteppedDecoding) stops the
    call once every row has finished, with the ids of the full run, and return_logp then returns the steps that ran,
    (last_steps_run, B, V). Training mode with an eos_id raises."""

    def __init__(self, model, max_tgt_len, multi_gpu=False, graph=False, constraints=None, eos_id=None,
                 early_stop=False):
        super().__init__(model, max_tgt_len, multi_gpu)
        self.eos_id = eos_id
        self._init_stepped(graph, early_stop, repeat_heads=True)  # as CSATrans.decode masks
        self.constraints = constraints

    def forward(self, data, return_logp=False):
        m = self.model
        if m.training:
            if self.constraints is not None or self.eos_id is not None:
                raise RuntimeError("CachedGreedyGenerator: constraints and eos_id are for inference only (the uncached "
                                   "loop that training mode defers to has neither)")
            ys = super().forward(data)
            self.last_steps_run = self.last_replays = self.max_tgt_len - 1
            return (ys, None) if return_logp else ys
        from .decode_ops import argmax_rows
        from .gen_ops import gen_log_softmax
        with torch.no_grad():
            m.process_data(data)
            enc, _, _, _, _ = m.encode(data)
            if self.graph and enc.is_cuda:
                return self._forward_graph(data, enc, return_logp)
            B, T = enc.size(0), self.max_tgt_len
            if self.eos_id is not None:  # the device-stepped step run eagerly, as the other two generators do
                e = self._state(m.decoder.make_cache(enc, data.src_mask, T, repeat_heads=True), bool(return_logp))
                self._reset(e)
                return self._decode(e, False)
            cache = m.decoder.make_cache(enc, data.src_mask, T, repeat_heads=True)  # as CSATrans.decode masks
            ys = torch.zeros(B, T, dtype=torch.long, device=enc.device)
            ys[:, 0] = self.start_pos
            logps = []
            con = self.constraints
            suppress = None if con is None else con.suppress_tensor(enc.device)
            for t in range(T - 1):
                x = m.tgt_embedding.step(ys[:, t:t + 1], t)
                dec = m.decoder.step(x, cache, t)
                logits = m.generator.linear(dec[:, 0])
                if con is not None:
                    con.apply(logits, ys, t, suppress=suppress)
                argmax_rows(logits, out=ys[:, t + 1], is_pad=cache.pad[:, t + 1], pad_id=PAD)
                if return_logp:
                    logps.append(gen_log_softmax(logits, 0.0))
            self.last_steps_run = self.last_replays = T - 1
            out = ys[:, 1:]
            return (out, torch.stack(logps)) if return_logp else out

    # ---- graph=True: the device-stepped decode step that _SteppedDecoding captures and replays ----

    def _state(self, cache, return_logp):
        """The static buffers beside the cache: tokens, the step counter, and the slot where each replay leaves its
        log-probabilities when return_logp asks for them."""
        B, T = cache.pad.shape
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=cache.pad.device)
        return SimpleNamespace(cache=cache, ys=z(B, T, dtype=torch.long), t_dev=z(1, dtype=torch.int32), logp=None,
                               return_logp=return_logp, suppress=self._suppress_state(cache.pad.device),
                               fin=z(B, dtype=torch.uint8) if self.eos_id is not None else None,
                               stop=self._stop_state(cache.pad.device), stop_host=None)

    def _device_step(self, e):
        """One decode step with every step-dependent index read from e.t_dev on the device: the same launches for
        every t, so they can be captured once. Ends by advancing the counter, after its last reader."""
        from .decode_ops import argmax_rows
        from .gen_ops import gen_log_softmax
        m = self.model
        x = m.tgt_embedding.step(e.ys, e.t_dev)
        dec = m.decoder.step(x, e.cache, e.t_dev)
        logits = m.generator.linear(dec[:, 0])
        if self.constraints is not None:  # with eos_id, a finished row takes PAD whatever its logits: left alone
            self.constraints.apply(logits, e.ys, e.t_dev, fin=e.fin, suppress=e.suppress)
        if e.fin is None:
            argmax_rows(logits, out=e.ys, is_pad=e.cache.pad, pad_id=PAD, t_dev=e.t_dev, head_pad=e.cache.head_pad)
        else:
            argmax_rows(logits, out=e.ys, is_pad=e.cache.pad, pad_id=PAD, t_dev=e.t_dev, head_pad=e.cache.head_pad,
                        fin=e.fin, eos_id=self.eos_id)
        e.logp = gen_log_softmax(logits, 0.0) if e.return_logp else None
        self._advance(e)

    def _reset(self, e):
        """Step 0 of a new batch. The self-attention cache needs no reset: rows above t are never read."""
        e.ys.zero_()
        e.ys[:, 0] = self.start_pos
        e.cache.pad.zero_()
        e.cache.head_pad.zero_()
        if e.fin is not None:
            e.fin.zero_()
        if e.stop is not None:
            e.stop.zero_()
        e.t_dev.zero_()

    def _eos_key(self):
        """What eos_id adds to the graph key extras: nothing without one."""
        return () if self.eos_id is None else ("eos", int(self.eos_id))

    def _forward_graph(self, data, enc, return_logp):
        return_logp = bool(return_logp)
        extras = (return_logp, *self._constraint_key(), *self._eos_key(), *self._stop_key())
        return self._decode(self._graph_entry(enc, data.src_mask, extras, return_logp=return_logp), True)

    def _decode(self, e, graphed):
        """The steps of one call on the reset state e; each step's log-probabilities are copied out of their slot as
        the step is issued, and those of the steps that ran are returned."""
        logps = []
        self._run_steps(e, graphed, (lambda: logps.append(e.logp.clone())) if e.return_logp else None)
        out = e.ys[:, 1:].clone()
        return (out, torch.stack(logps[:self.last_steps_run])) if e.return_logp else out


class BeamSearchGenerator(_SteppedDecoding, nn.Module):
    """Beam search of width W = beam_size over the KV-cached, device-stepped decode step (no counterpart in the
    reference, whose only strategy is GreedyGenerator).

    Rows are R = B * W hypotheses, row r = b * W + w. All max_tgt_len - 1 steps run (static shapes) unless
    early_stop=True (_SteppedDecoding) ends the call once every hypothesis has finished; the result is bitwise the same.
    cum (fp32) starts at 0 for row b * W and -inf for the other W - 1 rows, all tokens BOS. Per step the eval-mode
    generator logits z give logp = z - lse (fp32) and a candidate scores cum[r] + (z - lse[r]); a hypothesis that has
    emitted eos_id is finished (None: never), offers the single candidate (cum, PAD), and its row still runs through
    the decoder, ignored. Per AST the best W candidates survive: score descending, then parent row, then token.
    The self-attention key mask is the hypothesis' own PAD columns (make_std_mask per row, DecodeCache without
    repeat_heads): the reference decode()'s `.repeat(num_heads, 1, 1)` would let a finished hypothesis' padding mask
    keys of live ones, so it is not reproduced here.

    Nothing is gathered between steps: the K/V cache stays where each step stored it and the attention follows the
    (R, T) ancestry table that the selection rewrites (decode_ops.beam_row_topk / beam_select, decode_attention's anc=
    and kv_group=); the W hypotheses of an AST share one memory projection. The step index lives in a 4-byte device
    counter, so the launches of a step never depend on it.

    After the last step the W hypotheses of an AST are ranked by cum / len ** length_penalty, len counting tokens up
    to and including the first EOS (max_tgt_len - 1 without one). forward returns the best ids (B, max_tgt_len - 1),
    PAD after EOS; with return_all also the ids (B, W, max_tgt_len - 1) and scores (B, W) in rank order.

    graph=True (CUDA model): as CachedGreedyGenerator, the step is replayed from one captured graph per
    (..., beam_size, ...) (_SteppedDecoding); bitwise the eager result. Inference only: a model in training mode
    raises.

    constraints=DecodingConstraints(...): every live hypothesis' logits go through decode_ops.constrain_rows (its own
    history, as the selection rewrote it) before the row top-W; a banned token is a -inf logit, so lse and the scores
    are those of the distribution renormalised over what is left. Finished hypotheses are left alone."""

    def __init__(self, model, max_tgt_len, beam_size, length_penalty=0.0, eos_id=EOS, multi_gpu=False, graph=False,
                 constraints=None, early_stop=False):
        super().__init__()
        if not 1 <= beam_size <= 8:
            raise ValueError("BeamSearchGenerator: beam_size must be in [1, 8]")
        if max_tgt_len < 2:
            raise ValueError("BeamSearchGenerator: max_tgt_len must be at least 2")
        self.model = model.module if multi_gpu else model
        self.max_tgt_len = max_tgt_len
        self.beam_size = beam_size
        self.length_penalty = float(length_penalty)
        self.eos_id = eos_id
        self.start_pos = BOS
        self._init_stepped(graph, early_stop, beam=beam_size)
        self.constraints = constraints

    def forward(self, data, return_all=False):
        m = self.model
        self._check_eval()
        with torch.no_grad():
            m.process_data(data)
            enc, _, _, _, _ = m.encode(data)
            return self.search(enc, data.src_mask, return_all)

    def search(self, enc, src_mask=None, return_all=False):
        """The decoder side alone: enc (B, S, E) batch-first memory (any source, CPU included), src_mask (B, S) bool
        key-padding mask or None."""
        self._check_eval()
        V = self.model.generator.linear.weight.shape[0]
        if V < self.beam_size:
            raise ValueError("BeamSearchGenerator: the target vocabulary is smaller than the beam")
        with torch.no_grad():
            if self.graph and enc.is_cuda:
                e = self._graph_entry(enc, src_mask, (self.beam_size, *self._constraint_key(), *self._stop_key()))
                self._run_steps(e, True)
            else:
                cache = self.model.decoder.make_cache(enc, src_mask, self.max_tgt_len, beam=self.beam_size)
                e = self._state(cache)
                self._reset(e)
                self._run_steps(e, False)
            return self._rank(e, enc.size(0), return_all)

    def _check_eval(self):
        if self.model.training:
            raise RuntimeError("BeamSearchGenerator: inference only (the model is in training mode)")

    def _state(self, cache):
        """The per-hypothesis state beside the cache: tokens, cumulative log-probability, finished flag, the step
        counter and the row top-W buffers."""
        R, T, W, dev = cache.pad.shape[0], self.max_tgt_len, self.beam_size, cache.pad.device
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)
        return SimpleNamespace(cache=cache, ys=z(R, T, dtype=torch.long), cum=z(R, dtype=torch.float32),
                               fin=z(R, dtype=torch.uint8), t_dev=z(1, dtype=torch.int32),
                               lse=z(R, dtype=torch.float32), topv=z(R, W, dtype=torch.float32),
                               topi=z(R, W, dtype=torch.int32), suppress=self._suppress_state(dev),
                               stop=self._stop_state(dev), stop_host=None)

    def _reset(self, e):
        """Step 0 of a new batch: BOS everywhere, one live hypothesis per AST. The self-attention cache needs no
        reset (rows above t are never read); the ancestry table is cleared so that every entry stays a valid row."""
        e.ys.zero_()
        e.ys[:, 0] = self.start_pos
        e.cache.pad.zero_()
        e.cache.anc.zero_()
        e.cum.fill_(float("-inf"))
        e.cum.view(-1, self.beam_size)[:, 0] = 0.0
        e.fin.zero_()
        if e.stop is not None:
            e.stop.zero_()
        e.t_dev.zero_()

    def _device_step(self, e):
        """One beam step with every step-dependent index read from e.t_dev (on the device where the kernels run): the
        same launches for every t. Ends by advancing the counter, after its last reader."""
        from .decode_ops import beam_row_topk, beam_select
        m, T = self.model, self.max_tgt_len
        x = m.tgt_embedding.step(e.ys, e.t_dev)
        dec = m.decoder.step(x, e.cache, e.t_dev)
        logits = m.generator.linear(dec[:, 0])
        if self.constraints is not None:  # a finished hypothesis offers (cum, PAD) whatever its logits: left alone
            self.constraints.apply(logits, e.ys, e.t_dev, fin=e.fin, suppress=e.suppress)
        beam_row_topk(logits, self.beam_size, e.lse, e.topv, e.topi, t_dev=e.t_dev, t_end=T - 1)
        beam_select(e.topv, e.topi, e.lse, e.cum, e.fin, e.ys, e.cache.pad, e.cache.anc, e.t_dev, eos_id=self.eos_id,
                    pad_id=PAD)
        self._advance(e)

    def _rank(self, e, B, return_all):
        W, T = self.beam_size, self.max_tgt_len
        ids = e.ys[:, 1:]
        length = torch.full((B * W,), T - 1, dtype=torch.long, device=ids.device)
        if self.eos_id is not None:
            is_eos = ids == self.eos_id
            length = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, length)
        score = e.cum.clone() if self.length_penalty == 0.0 else e.cum / length.float() ** self.length_penalty
        score = score.view(B, W)
        order = torch.argsort(score, dim=1, descending=True, stable=True)
        ranked = ids.reshape(B, W, T - 1).gather(1, order[:, :, None].expand(B, W, T - 1))
        best = ranked[:, 0].clone()
        return (best, ranked, score.gather(1, order)) if return_all else best

    def _check_capture(self, enc):
        from ._lib import lib
        if not lib().csa_beam_supported(self.beam_size, self.max_tgt_len) or enc.dtype != torch.float32:
            raise ValueError("BeamSearchGenerator: graph=True needs fp32 and max_tgt_len <= 256 (csa_beam_supported)")
        self._check_constraints_capture(enc)


class SamplingGenerator(_SteppedDecoding, nn.Module):
    """Sampled decoding over the KV-cached, device-stepped decode step: num_samples independent draws per AST from the
    model's distribution, filtered by temperature, top_k (0: off) and top_p (>= 1: off), with the log-probability of
    every drawn token (no counterpart in the reference, whose only strategy is GreedyGenerator).

    Rows are R = B * num_samples, row r = b * num_samples + s. Each row keeps its own self-attention cache row (no
    ancestry table); the rows of an AST share one memory projection and mask (DecodeCache kv_group, make_cache's
    group=). The self-attention key mask is the row's own PAD columns, as in BeamSearchGenerator and for its reason:
    the reference decode()'s `.repeat(num_heads, 1, 1)` would let a finished sample's padding mask keys of live ones.
    Per step the eval-mode generator logits go through decode_ops.sample_rows (csrc/csa_sample.hip): y = z /
    temperature, top-k with all ties, top-p on the renormalised top-k set (tie-inclusive), one Gumbel-max draw from
    Philox stream 7 keyed by (seed, row, step, column), logp = y[token] - lse(y over the kept set). A row that has
    emitted eos_id is finished (None: never): it takes PAD with logp 0 and still runs through the decoder, ignored.
    All max_tgt_len - 1 steps run (static shapes) unless early_stop=True (_SteppedDecoding) ends the call once every row
    has finished; ids and log-probabilities are bitwise the same.

    forward(data, seed=None, return_logp=False) / sample(enc, src_mask, seed, return_logp) return the ids
    (B, max_tgt_len - 1), or (B, num_samples, max_tgt_len - 1) when num_samples > 1, PAD after EOS; with return_logp
    also the per-token log-probabilities of the same shape, 0 after EOS, whose sum over the last dim is the sequence
    log-probability under the sampled (filtered) distribution. seed: a 64-bit key; None draws one from torch's CPU
    generator (reproducible under torch.manual_seed). The same seed repeats the same draws on any device path.

    graph=True (CUDA model): as CachedGreedyGenerator, the step is replayed from one captured graph per
    (..., temperature, top_k, top_p, num_samples, eos_id, return_logp, ...) (_SteppedDecoding); the seed lives in a
    16-byte device buffer filled outside the graph, so a replay draws anew. Bitwise the eager result. Inference only:
    a model in training mode raises.

    constraints=DecodingConstraints(...): every live row's logits go through decode_ops.constrain_rows before
    sample_rows, which never draws a -inf entry and renormalises: logp is the log-probability under the constrained,
    filtered distribution. Finished rows are left alone."""

    def __init__(self, model, max_tgt_len, temperature=1.0, top_k=0, top_p=1.0, num_samples=1, eos_id=EOS,
                 multi_gpu=False, graph=False, constraints=None, early_stop=False):
        super().__init__()
        if not float(temperature) > 0.0:
            raise ValueError("SamplingGenerator: temperature must be positive")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError("SamplingGenerator: top_k must be a non-negative integer (0 turns it off)")
        if not float(top_p) > 0.0:
            raise ValueError("SamplingGenerator: top_p must be positive (1 or more turns it off)")
        if int(num_samples) != num_samples or num_samples < 1:
            raise ValueError("SamplingGenerator: num_samples must be a positive integer")
        if max_tgt_len < 2:
            raise ValueError("SamplingGenerator: max_tgt_len must be at least 2")
        self.model = model.module if multi_gpu else model
        self.max_tgt_len = max_tgt_len
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.num_samples = int(num_samples)
        self.eos_id = eos_id
        self.start_pos = BOS
        self._init_stepped(graph, early_stop, group=self.num_samples)
        self.constraints = constraints

    def forward(self, data, seed=None, return_logp=False):
        m = self.model
        self._check_eval()
        with torch.no_grad():
            m.process_data(data)
            enc, _, _, _, _ = m.encode(data)
            return self.sample(enc, data.src_mask, seed, return_logp)

    def sample(self, enc, src_mask=None, seed=None, return_logp=False):
        """The decoder side alone: enc (B, S, E) batch-first memory (any source, CPU included), src_mask (B, S) bool
        key-padding mask or None."""
        self._check_eval()
        return_logp = bool(return_logp)
        if seed is None:  # one 64-bit Philox key per call from torch's global CPU generator, as ops._draw_seed
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        key = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed, 0], dtype=torch.int64)  # {seed, offset}
        T = self.max_tgt_len
        with torch.no_grad():
            if self.graph and enc.is_cuda:
                extras = (self.temperature, self.top_k, self.top_p, self.num_samples, self.eos_id, return_logp,
                          *self._constraint_key(), *self._stop_key())
                e = self._graph_entry(enc, src_mask, extras, return_logp=return_logp)
                e.rng.copy_(key)  # outside the graph: the replays read it on the device
                self._run_steps(e, True)
            else:
                cache = self.model.decoder.make_cache(enc, src_mask, T, group=self.num_samples)
                e = self._state(cache, return_logp)
                self._reset(e)
                e.rng.copy_(key)
                self._run_steps(e, False)
            shape = (enc.size(0), T - 1) if self.num_samples == 1 else (enc.size(0), self.num_samples, T - 1)
            ids = e.ys[:, 1:].reshape(shape).clone()
            return (ids, e.logp.reshape(shape).clone()) if return_logp else ids

    def _check_eval(self):
        if self.model.training:
            raise RuntimeError("SamplingGenerator: inference only (the model is in training mode)")

    def _state(self, cache, return_logp):
        """The per-row state beside the cache: tokens, finished flag, the step counter, the {seed, offset} key that the
        kernel reads on the device and, when asked for, the per-token log-probabilities."""
        R, T, dev = cache.pad.shape[0], self.max_tgt_len, cache.pad.device
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)
        return SimpleNamespace(cache=cache, ys=z(R, T, dtype=torch.long), fin=z(R, dtype=torch.uint8),
                               t_dev=z(1, dtype=torch.int32), rng=z(2, dtype=torch.int64),
                               logp=z(R, T - 1, dtype=torch.float32) if return_logp else None,
                               suppress=self._suppress_state(dev), stop=self._stop_state(dev), stop_host=None)

    def _reset(self, e):
        """Step 0 of a new batch: BOS everywhere, no row finished. The self-attention cache needs no reset (rows above t
        are never read)."""
        e.ys.zero_()
        e.ys[:, 0] = self.start_pos
        e.cache.pad.zero_()
        e.fin.zero_()
        if e.logp is not None:
            e.logp.zero_()
        if e.stop is not None:
            e.stop.zero_()
        e.t_dev.zero_()

    def _device_step(self, e):
        """One sampling step with every step-dependent index read from e.t_dev (on the device where the kernels run):
        the same launches for every t. Ends by advancing the counter, after its last reader."""
        from .decode_ops import sample_rows
        m = self.model
        x = m.tgt_embedding.step(e.ys, e.t_dev)
        dec = m.decoder.step(x, e.cache, e.t_dev)
        logits = m.generator.linear(dec[:, 0])
        if self.constraints is not None:  # a finished row takes PAD whatever its logits: left alone
            self.constraints.apply(logits, e.ys, e.t_dev, fin=e.fin, suppress=e.suppress)
        sample_rows(logits, e.ys, e.cache.pad, e.fin, e.t_dev, e.rng, temperature=self.temperature, top_k=self.top_k,
                    top_p=self.top_p, eos_id=self.eos_id, pad_id=PAD, logp=e.logp)
        self._advance(e)

    def _check_capture(self, enc):
        from ._lib import lib
        V = self.model.generator.linear.weight.shape[0]
        if not lib().csa_sample_rows_supported(V) or enc.dtype != torch.float32:
            raise ValueError("SamplingGenerator: graph=True needs fp32 and a target vocabulary of at most 32768 "
                             "(csa_sample_rows_supported)")
        self._check_constraints_capture(enc)


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
