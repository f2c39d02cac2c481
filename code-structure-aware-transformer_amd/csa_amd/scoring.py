"""Scoring GIVEN summaries under the model (no counterpart in the reference beyond ignite's Loss next to BLEU4):
teacher-forced log-probabilities of candidate ids, re-ranking by them, and validation NLL / perplexity.

One full decoder pass over [BOS, candidate[:-1]], the generator's linear, and score_ops.token_logp (csrc/csa_score.hip),
which keeps logit[target] - logsumexp per position and never materialises the (rows, V) log-probabilities. The names of
this module are re-exported by csa_amd.model."""
import math
from types import SimpleNamespace

import torch
import torch.nn as nn

from .data import BOS, EOS
from .model import PAD, make_std_mask
from .score_ops import token_logp

HEAD_MASKS = ("own", "reference")
ATTENTIONS = ("sdpa", "fused")


class SequenceScorer(nn.Module):
    """log p(candidate | AST) under `model`, teacher-forced: the decoder reads [BOS, candidate[:, :-1]] and position t
    is scored on candidate[:, t]. Candidates are ids WITHOUT BOS, (B, T') or (B, G, T') int64, exactly what the
    generators return (a beam's return_all list, a sampler's num_samples rows), G candidates per AST.

    Which positions are scored: with eos_id, every position up to and including the first eos_id (whatever follows
    gets log-probability 0, as the generators write PAD there); with eos_id=None every non-PAD position.

    The logits are model.generator.linear(decoder output) alone: the Generator's dropout on the logits is NOT applied,
    in any mode, and the log-probability is a true log-softmax, finite where the Generator's log(softmax) underflows to
    -inf. The rest of the model runs in whatever mode it is in (eval mode is not required; in training mode the
    embedding and decoder dropouts are active). Under enabled gradients the result is differentiable: gradients reach
    the generator, decoder and, through forward(), the encoder. No host sync.

    head_mask, the self-attention key mask of the decoder:
      "own"        head h of row r sees row r's own PAD columns, the (R * H, T, T) mask built by repeat_interleave, as
                   BeamSearchGenerator and SamplingGenerator mask: a row's score does not depend on its batch
                   neighbours, and equals what those generators accumulated.
      "reference"  make_std_mask(...).repeat(H, 1, 1) as CSATrans.decode passes it, which nn.MultiheadAttention reads
                   as (R, H, T, T): head h of row r sees the PAD columns of row (r * H + h) % R. These are the
                   training forward's numbers (and CachedGreedyGenerator's).

    forward(data, candidates, return_tokens=False) runs process_data + encode once per AST; score(enc, src_mask,
    candidates, return_tokens=False) starts from a precomputed memory (B, S, E), any device, CPU included (the decoder's
    torch paths and the op's fallback). Both return namespace(logp (B, G) fp32 sums over the scored positions, length
    (B, G) int32 counts of them, tokens (B, G, T') fp32 per-position log-probabilities or None); G is squeezed away for
    (B, T') input. The sum is a plain sum(-1) of the per-token vector: deterministic.

    attention, how the decoder pass runs:
      "sdpa"   decoder.forward(): torch SDPA with float masks (R * H, T, T) and (R * H, 1, S); with G > 1 candidates
               per AST the memory and its mask are repeated G times, so every layer projects B * G * S memory rows.
      "fused"  decoder.forward_fused() on seq_attn_ops.seq_attention (csrc/csa_seqattn.hip): the masks are read in
               the kernel from the (R, T) PAD bytes and the (B, S) memory mask, and the G rows of an AST read ONE memory
               projection (kv_group = G), their dK / dV summed in the kernel. No float mask, no repeated memory. The
               kernel has no attention dropout: a decoder in training mode with dropout > 0 runs its attention calls on
               SDPA with the distribution of "sdpa" (still without the repeated projection).
    last_attention: "fused" when every attention of the last call ran the fused op, else "sdpa"; None before a call."""

    def __init__(self, model, eos_id=EOS, head_mask="own", multi_gpu=False, attention="sdpa"):
        super().__init__()
        if attention not in ATTENTIONS:
            raise ValueError(f"SequenceScorer: attention must be one of {ATTENTIONS}")
        self.attention = attention
        self.last_attention = None
        if head_mask not in HEAD_MASKS:
            raise ValueError(f"SequenceScorer: head_mask must be one of {HEAD_MASKS}")
        if eos_id is not None and (isinstance(eos_id, bool) or int(eos_id) != eos_id or eos_id < 0):
            raise ValueError("SequenceScorer: eos_id must be a non-negative integer or None")
        self.model = model.module if multi_gpu else model
        self.eos_id = None if eos_id is None else int(eos_id)
        self.head_mask = head_mask
        self.start_pos = BOS

    def forward(self, data, candidates, return_tokens=False):
        m = self.model
        m.process_data(data)
        return self.score(m.encode(data)[0], data.src_mask, candidates, return_tokens)

    def score(self, enc, src_mask, candidates, return_tokens=False):
        if candidates.dtype != torch.int64 or candidates.dim() not in (2, 3) or candidates.shape[0] != enc.shape[0]:
            raise ValueError("SequenceScorer: candidates must be int64 ids (B, T') or (B, G, T') for a (B, S, E) memory")
        squeeze = candidates.dim() == 2
        B, G, T = enc.shape[0], 1 if squeeze else candidates.shape[1], candidates.shape[-1]
        cand = candidates.reshape(B * G, T)
        bos = torch.full((B * G, 1), self.start_pos, dtype=torch.int64, device=cand.device)
        dec_in = torch.cat([bos, cand[:, :-1]], 1)
        if self.eos_id is None:
            scored = cand != PAD
        else:  # up to and including the first EOS: no EOS strictly before the position
            is_eos = (cand == self.eos_id).to(torch.int32)
            scored = (is_eos.cumsum(1) - is_eos) == 0
        tokens = self.token_logps(enc, src_mask, dec_in, cand, scored, G)
        out_shape = (B,) if squeeze else (B, G)
        return SimpleNamespace(logp=tokens.sum(-1).view(out_shape),
                               length=scored.sum(-1, dtype=torch.int32).view(out_shape),
                               tokens=tokens.view(*out_shape, T) if return_tokens else None)

    def token_logps(self, enc, src_mask, dec_in, target, scored, group=1):
        """The teacher-forced pass itself: memory enc (B, S, E) and its key-padding mask (B, S) bool or None, decoder
        input ids dec_in (B * group, T), targets (B * group, T) and the bool mask of the positions to score ->
        (B * group, T) fp32 log-probabilities, 0 where not scored."""
        m = self.model
        if self.attention == "fused":
            dec = m.decoder.forward_fused(m.tgt_embedding(dec_in), enc, (dec_in == PAD).to(torch.uint8),
                                          None if src_mask is None else src_mask.to(torch.uint8),
                                          mask_mode=self.head_mask, kv_group=group)
            self.last_attention = "fused" if m.decoder.last_fused else "sdpa"
            logits = m.generator.linear(dec)
            return token_logp(logits, torch.where(scored, target, torch.full_like(target, -1)), ignore_id=-1)
        self.last_attention = "sdpa"
        H = m.decoder.layers[0].self_attn.num_heads
        mask = make_std_mask(dec_in, PAD)
        tgt_mask = mask.repeat(H, 1, 1) if self.head_mask == "reference" else mask.repeat_interleave(H, 0)
        if group > 1:
            enc = enc.repeat_interleave(group, 0)
            src_mask = None if src_mask is None else src_mask.repeat_interleave(group, 0)
        dec, _ = m.decoder(m.tgt_embedding(dec_in).permute(1, 0, 2), enc.permute(1, 0, 2), tgt_mask=tgt_mask,
                           memory_key_padding_mask=src_mask)
        logits = m.generator.linear(dec.permute(1, 0, 2))
        # an unscored position becomes target -1, which token_logp ignores (0, and a zero gradient row)
        return token_logp(logits, torch.where(scored, target, torch.full_like(target, -1)), ignore_id=-1)


def rerank(ids, out, length_penalty=0.0):
    """Orders the G candidates of every AST by the model's own score: ids (B, G, T') as scored, out the namespace a
    SequenceScorer returned for them -> (best (B, T'), order (B, G) int64), order[b] the candidate indices by
    out.logp / out.length ** length_penalty descending (0: the plain sum), ties to the lower index. On ids' device, no
    host sync."""
    if ids.dim() != 3 or out.logp.shape != ids.shape[:2]:
        raise ValueError("rerank: ids (B, G, T') and the scores (B, G) of a SequenceScorer call on them")
    score = out.logp
    if length_penalty != 0.0:
        score = score / out.length.clamp(min=1).to(score.dtype) ** float(length_penalty)
    order = torch.argsort(score, dim=1, descending=True, stable=True)
    best = ids.gather(1, order[:, :1, None].expand(-1, 1, ids.shape[2]))[:, 0]
    return best, order


def validation_nll(model, batches, head_mask="reference", attention="sdpa"):
    """Token-level negative log-likelihood and perplexity over (data, target) batches: data.tgt_seq is the decoder input
    and the non-PAD positions of target (B, T) are scored, so with head_mask="reference" this is the number
    label_smoothing_loss(model(data)[0], target) reports at smoothing 0 for one batch, wherever that one is finite,
    pooled over all tokens of all batches. -> namespace(nll, ppl, tokens): Python floats and the token count. The
    log-probabilities are summed in fp64 on the device; one host sync, at the end. Runs under no_grad in the model's
    current mode (call model.eval() first for validation). attention: as SequenceScorer takes it."""
    scorer = SequenceScorer(model, eos_id=None, head_mask=head_mask, attention=attention)
    m = scorer.model
    total = count = None
    with torch.no_grad():
        for data, target in batches:
            m.process_data(data)
            enc = m.encode(data)[0]
            scored = target != PAD
            tok = scorer.token_logps(enc, data.src_mask, data.tgt_seq, target, scored)
            s, n = tok.sum(dtype=torch.float64), scored.sum()
            total, count = (s, n) if total is None else (total + s, count + n)
    if total is None:
        return SimpleNamespace(nll=float("nan"), ppl=float("nan"), tokens=0)
    total, count = torch.stack([total, count.to(torch.float64)]).tolist()
    nll = -total / count if count else float("nan")
    try:
        ppl = math.exp(nll)
    except OverflowError:
        ppl = float("inf")
    return SimpleNamespace(nll=nll, ppl=ppl, tokens=int(count))
