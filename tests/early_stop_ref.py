"""Oracles and cases of the early stop at EOS (csa_amd.decoding._SteppedDecoding, decode_ops.decode_advance and the
finished-flag form of argmax_rows), test infrastructure only.

steps_rule restates the stopping rule on an oracle's record of finished flags; greedy_eos_ref is the uncached greedy
loop with a finished flag (BaseDecoder.forward per step over all positions so far, the reference decode()'s
make_std_mask(...).repeat(H, 1, 1), finished rows forced to PAD, every step run); advance_np and argmax_fin_np restate the
two kernels in numpy. The beam and sampling oracles are tests/beam_ref.py and tests/sample_ref.py, run for all steps."""
import numpy as np
import torch

from beam_ref import BOS, EOS_ID, PAD  # noqa: F401 (shared with the tests)
from golden_inputs import fill_params_deterministic

# the decoder side of the tiny model of tests/golden/greedy_tiny.npz (the dims of test_beam_gpu.TINY)
TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            use_pegen="pegen", dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512,
            clusters=[10, 12], full_att=False)
T = 16

# fill_params_deterministic seed, generator scale and EOS bias. NEVER is test_beam_gpu.TINY_BEAM, in which some
# hypothesis is live at every step; with the EOS bias at 6.0 every hypothesis of the beam has finished after step 2.
BEAM_STOPS = dict(seed=6, gen_scale=24.0, eos_bias=6.0)
NEVER = dict(seed=6, gen_scale=24.0, eos_bias=2.0)
SAMPLING = dict(top_k=10, top_p=0.9)
SAMPLING_SEED = 1234
# the greedy case, chosen on greedy_eos_ref alone (seeds 1..12 x scales 8 and 24 x EOS biases 0.5 .. 6.0 in steps of
# 0.5): the only one whose rows finish at two or more distinct steps, all of them by step T - 4 (steps 4, 0 and 5)
GREEDY = dict(seed=2, gen_scale=8.0, eos_bias=6.0)
GREEDY_GAP = 1e-3  # the least top-2 logit gap of a live row that the greedy case must show (fp32 logits of size ~10)


def tiny_model(seed, gen_scale, eos_bias=0.0):
    from csa_amd.model import CSATrans
    m = CSATrans(**TINY)
    fill_params_deterministic(m, seed)
    with torch.no_grad():
        m.generator.linear.weight.mul_(gen_scale)
        m.generator.linear.bias[EOS_ID] += eos_bias
    return m.eval()


def tiny_memory(seed, device="cpu"):
    """A random memory of 3 ASTs and 20 source keys, two of them padded (the masks of test_beam_gpu._tiny_beam_case)."""
    enc = torch.randn(3, 20, 64, generator=torch.Generator().manual_seed(seed))
    src_mask = torch.zeros(3, 20, dtype=torch.bool)
    src_mask[1, 17:] = True
    src_mask[2, 12:] = True
    return enc.to(device), src_mask.to(device)


def tiny_case(case, mem_seed=None, device="cpu"):
    """The model of `case` with tiny_memory(mem_seed); mem_seed defaults to the model's seed, as in test_beam_gpu."""
    return (tiny_model(**case).to(device), *tiny_memory(case["seed"] if mem_seed is None else mem_seed, device))


class FixedMemory(torch.nn.Module):
    """The decoder side of a model behind the interface CachedGreedyGenerator.forward asks for, the encoder replaced by
    a fixed memory (the encoder's attention has no CPU path, and the decode loop is what is under test)."""

    def __init__(self, model, enc, src_mask):
        super().__init__()
        self.tgt_embedding, self.decoder, self.generator = model.tgt_embedding, model.decoder, model.generator
        self.enc, self.src_mask = enc, src_mask
        self.eval()

    def process_data(self, data):
        data.src_mask = self.src_mask

    def encode(self, data):
        return self.enc, 1, None, [], []


def steps_rule(fins, steps):
    """steps_run of the rule on a record of finished flags, fins[s] = the flags of every row after step s: s + 2 for
    the first s with all of them set, at most `steps`; `steps` without one."""
    for s in range(steps):
        if bool(np.asarray(fins[s]).all()):
            return min(s + 2, steps)
    return steps


def greedy_eos_ref(model, enc, src_mask, T, eos_id):
    """-> ids (B, T-1) int64, fins (T-1, B) bool, the finished flags after each step, and min_gap, the smallest
    difference between the two largest logits of a live row at any step."""
    from csa_amd.model import make_std_mask
    B = enc.shape[0]
    H = model.decoder.layers[0].self_attn.num_heads
    mem = enc.permute(1, 0, 2)
    ys = torch.full((B, 1), BOS, dtype=torch.long, device=enc.device)
    fin = torch.zeros(B, dtype=torch.bool, device=enc.device)
    fins, min_gap = [], float("inf")
    with torch.no_grad():
        for _ in range(T - 1):
            tgt_mask = make_std_mask(ys, PAD).repeat(H, 1, 1)
            dec, _ = model.decoder(model.tgt_embedding(ys).permute(1, 0, 2), mem, tgt_mask, memory_key_padding_mask=src_mask)
            z = model.generator.linear(dec.permute(1, 0, 2)[:, -1])
            top2 = z.float().topk(2, dim=1)[0]
            if bool((~fin).any()):
                min_gap = min(min_gap, float((top2[:, 0] - top2[:, 1])[~fin].min()))
            tok = torch.where(fin, torch.full_like(fin, PAD, dtype=torch.long), z.argmax(1))
            fin = fin | (tok == eos_id)
            ys = torch.cat([ys, tok[:, None]], dim=1)
            fins.append(fin.clone())
    return ys[:, 1:], torch.stack(fins), min_gap


def advance_np(fin, t, state, T):
    """k_decode_advance on numpy values -> (t, state) after the launch."""
    all_prev, steps, parked, reserved = (int(v) for v in state)
    if parked:
        return t, [all_prev, steps, parked, reserved]
    steps += 1
    if all_prev or t + 1 >= T - 1:
        return -1, [all_prev, steps, 1, reserved]
    return t + 1, [int(bool((np.asarray(fin) != 0).all())), steps, 0, reserved]


def argmax_fin_np(x, fin, eos_id, pad_id=PAD):
    """One finished-flag argmax step -> (tokens, PAD bytes, fin after)."""
    fin = np.asarray(fin, dtype=np.uint8)
    done = fin != 0
    tok = np.where(done, pad_id, np.asarray(x).argmax(axis=1)).astype(np.int64)  # the first maximal entry
    new_fin = np.where(~done & (tok == eos_id), 1, fin).astype(np.uint8)
    return tok, (tok == pad_id).astype(np.uint8), new_fin
