"""Plain-torch oracle of BeamSearchGenerator, uncached: every step re-runs BaseDecoder.forward over all R = B * W
hypotheses so far (make_std_mask per row, the memory repeated W times), takes log_softmax of the last position's
generator logits and selects with one stable descending sort over (row, token). Also numpy restatements of one
selection step and of the row top-W, for the hand-built states of the kernel tests."""
from types import SimpleNamespace

import numpy as np
import torch

PAD, BOS = 0, 2


def beam_search_ref(model, enc, src_mask, T, W, eos_id, length_penalty=0.0):
    """model: anything with tgt_embedding, decoder (BaseDecoder) and generator.linear, in eval mode.
    Returns a namespace: best (B, T-1), ids (B, W, T-1) and scores (B, W) in rank order, and of the run itself
    parents (T-1, B, W) local parent indices, fin (T-1, B, W) finished flags after each step, cum (T-1, B, W), and
    min_gap, the smallest difference between neighbours among the W + 1 best candidates of any AST at any step (the
    W-th against the (W+1)-th decides who survives, the others the order inside the beam)."""
    from csa_amd.model import make_std_mask
    B, S, E = enc.shape
    R, dev = B * W, enc.device
    H = model.decoder.layers[0].self_attn.num_heads
    mem = enc.repeat_interleave(W, 0).permute(1, 0, 2)
    mm = None if src_mask is None else src_mask.repeat_interleave(W, 0)
    ys = torch.full((R, 1), BOS, dtype=torch.long, device=dev)
    cum = torch.full((B, W), float("-inf"), device=dev)
    cum[:, 0] = 0.0
    fin = torch.zeros(B, W, dtype=torch.bool, device=dev)
    parents, fins, cums, min_gap = [], [], [], float("inf")
    with torch.no_grad():
        for _ in range(T - 1):
            tgt_mask = make_std_mask(ys, PAD).repeat_interleave(H, 0)
            dec, _ = model.decoder(model.tgt_embedding(ys).permute(1, 0, 2), mem, tgt_mask, memory_key_padding_mask=mm)
            z = model.generator.linear(dec.permute(1, 0, 2)[:, -1])
            logp = torch.log_softmax(z.float(), dim=-1).view(B, W, -1)
            V = logp.shape[-1]
            cand = cum[:, :, None] + logp
            done = torch.full_like(cand, float("-inf"))
            done[:, :, PAD] = cum
            cand = torch.where(fin[:, :, None], done, cand).view(B, W * V)
            v, i = torch.sort(cand, dim=1, descending=True, stable=True)
            gaps = (v[:, :W] - v[:, 1:W + 1]).flatten()
            gaps = gaps[torch.isfinite(gaps)]
            if gaps.numel():
                min_gap = min(min_gap, float(gaps.min()))
            par, tok = i[:, :W] // V, i[:, :W] % V
            prow = (par + W * torch.arange(B, device=dev)[:, None]).reshape(R)
            ys = torch.cat([ys[prow], tok.reshape(R, 1)], dim=1)
            fin = fin.gather(1, par)
            if eos_id is not None:
                fin = fin | (tok == eos_id)
            cum = v[:, :W].clone()
            parents.append(par)
            fins.append(fin)
            cums.append(cum)
    ids = ys[:, 1:]
    length = torch.full((R,), T - 1, dtype=torch.long, device=dev)
    if eos_id is not None:
        is_eos = ids == eos_id
        length = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, length)
    score = (cum.reshape(R) / length.float() ** length_penalty).view(B, W)
    order = torch.argsort(score, dim=1, descending=True, stable=True)
    ranked = ids.view(B, W, T - 1).gather(1, order[:, :, None].expand(B, W, T - 1))
    return SimpleNamespace(best=ranked[:, 0], ids=ranked, scores=score.gather(1, order), parents=torch.stack(parents),
                           fin=torch.stack(fins), cum=torch.stack(cums), min_gap=min_gap)


def row_topk_np(z, W):
    """(lse fp64, topv, topi) of each row of z: a stable descending sort, the lowest index first among equals."""
    z = np.asarray(z, dtype=np.float64)
    order = np.argsort(-z, axis=1, kind="stable")[:, :W]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = z.max(axis=1)
        lse = np.where(np.isfinite(m), m + np.log(np.exp(z - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(axis=1)), m)
    return lse, np.take_along_axis(z, order, axis=1), order.astype(np.int32)


def select_np(topv, topi, lse, cum, fin, tokens, pad, anc, t, eos_id, pad_id=PAD):
    """One selection step on copies of the state, in the rule's own words: returns (cum, fin, tokens, pad, anc,
    parent). Scores are formed in fp32, cum + (z - lse), as the kernel forms them."""
    topv, lse, cum = (np.asarray(x, dtype=np.float32) for x in (topv, lse, cum))
    R, W = topv.shape
    cum2, fin2 = cum.copy(), np.array(fin, dtype=np.uint8)
    tok2, pad2, anc2 = np.array(tokens), np.array(pad), np.array(anc)
    parent = np.zeros(R, dtype=np.int32)
    for b in range(R // W):
        cands = []
        for w in range(W):
            r = b * W + w
            if fin[r]:
                cands.append((cum[r], w, pad_id))
            else:
                for k in range(W):
                    with np.errstate(invalid="ignore"):
                        cands.append((np.float32(cum[r] + np.float32(topv[r, k] - lse[r])), w, int(topi[r, k])))
        cands = [(s if s > -np.inf else np.float32(-np.inf), w, tk) for s, w, tk in cands]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        for c, (s, w, tk) in enumerate(cands[:W]):
            r, p = b * W + c, b * W + w
            tok2[r, :t + 1] = tokens[p, :t + 1]
            pad2[r, :t + 1] = pad[p, :t + 1]
            anc2[r, :t] = anc[p, :t]
            tok2[r, t + 1], pad2[r, t + 1], anc2[r, t] = tk, int(tk == pad_id), p
            cum2[r] = s
            fin2[r] = 1 if (fin[p] or (eos_id is not None and tk == eos_id)) else 0
            parent[r] = p
    return cum2, fin2, tok2, pad2, anc2, parent


# ---- hand-built selection states (shared by the CPU fallback test and the GPU kernel test) ----

EOS_ID, TOK_FILL, PAD_FILL, ANC_FILL = 3, 99, 7, -5


def _base_state(W, T, t, B, seed):
    """B ASTs with a random history up to column t (sentinels above it) and generic live rows."""
    g = np.random.default_rng(seed)
    R = B * W
    tokens = np.full((R, T), TOK_FILL, dtype=np.int64)
    pad = np.full((R, T), PAD_FILL, dtype=np.uint8)
    anc = np.full((R, T), ANC_FILL, dtype=np.int32)
    tokens[:, :t + 1] = g.integers(4, 50, size=(R, t + 1))
    tokens[:, 0] = BOS
    pad[:, :t + 1] = 0
    anc[:, :t] = (np.arange(R)[:, None] // W) * W + g.integers(0, W, size=(R, t))
    topv = -np.sort(-g.normal(size=(R, W)).astype(np.float32), axis=1)
    topi = np.stack([g.permutation(np.arange(4, 60))[:W] for _ in range(R)]).astype(np.int32)
    lse = (topv[:, 0] + np.float32(0.5)).astype(np.float32)
    cum = -g.uniform(1.0, 3.0, size=R).astype(np.float32)
    fin = np.zeros(R, dtype=np.uint8)
    return dict(W=W, T=T, t=t, eos_id=EOS_ID, topv=topv, topi=topi, lse=lse, cum=cum, fin=fin, tokens=tokens, pad=pad,
                anc=anc)


def select_states():
    """(name, state, claim): claim(parent, fin, tokens, pad) asserts that AST 0 of the EXPECTED result shows the
    situation the name promises (AST 1 is a generic state, so more than one workgroup runs)."""
    out = []
    s = _base_state(3, 6, 0, 2, 1)
    s["cum"][:] = [0, -np.inf, -np.inf, 0, -np.inf, -np.inf]
    out.append(("step0_one_finite_cum", s, lambda p, f, tk, pd: list(p[:3]) == [0, 0, 0]))
    s = _base_state(3, 6, 3, 2, 2)
    s["fin"][1], s["cum"][:3] = 1, [-1.0, -0.5, -3.0]
    s["tokens"][1, 2:4], s["pad"][1, 3] = [EOS_ID, PAD], 1
    out.append(("finished_row_stays", s,
                lambda p, f, tk, pd: p[0] == 1 and f[0] == 1 and tk[0, 4] == PAD and pd[0, 4] == 1 and pd[0, 3] == 1))
    s = _base_state(3, 6, 3, 2, 3)
    s["fin"][1], s["cum"][:3] = 1, [-1.0, -50.0, -1.2]
    out.append(("finished_row_falls_out", s, lambda p, f, tk, pd: 1 not in list(p[:3]) and not f[:3].any()))
    s = _base_state(3, 6, 2, 2, 4)
    s["cum"][:3] = [-0.1, -9.0, -9.0]
    s["topv"][0], s["lse"][0] = [1.0, 0.9, 0.8], 1.5
    out.append(("one_parent_two_children", s, lambda p, f, tk, pd: list(p[:3]) == [0, 0, 0]))
    s = _base_state(2, 6, 2, 2, 5)
    s["cum"][:2] = [-2.0, -1.0]
    s["topv"][:2], s["lse"][:2] = [[5.0, 0.0], [5.0, 0.0]], 5.5
    out.append(("pure_swap_of_rows_0_and_1", s, lambda p, f, tk, pd: list(p[:2]) == [1, 0]))
    s = _base_state(3, 6, 2, 2, 6)
    s["cum"][:3] = -1.0
    s["topv"][:3], s["lse"][:3] = [[2.0, 2.0, 0.0], [2.0, 1.0, 0.0], [2.0, 1.0, 0.0]], 2.5
    s["topi"][:3] = [[4, 9, 7], [3, 9, 1], [5, 6, 8]]
    out.append(("score_ties_row_then_token", s,
                lambda p, f, tk, pd: list(p[:3]) == [0, 0, 1] and list(tk[:3, 3]) == [4, 9, 3]))
    s = _base_state(3, 6, 2, 2, 7)
    s["cum"][:3] = [-0.1, -9.0, -9.0]
    s["topv"][0], s["lse"][0], s["topi"][0] = [3.0, 0.0, -1.0], 3.2, [EOS_ID, 8, 9]
    out.append(("token_equal_to_eos", s, lambda p, f, tk, pd: tk[0, 3] == EOS_ID and f[0] == 1 and pd[0, 3] == 0))
    s = _base_state(3, 6, 2, 2, 8)
    s["cum"][:3] = [-0.1, -9.0, -9.0]
    s["topv"][0], s["lse"][0], s["topi"][0] = [3.0, 0.0, -1.0], 3.2, [PAD, 8, 9]
    out.append(("live_hypothesis_emits_pad", s, lambda p, f, tk, pd: tk[0, 3] == PAD and pd[0, 3] == 1 and f[0] == 0))
    s = _base_state(4, 6, 4, 2, 9)
    out.append(("t_at_T_minus_2", s, lambda p, f, tk, pd: bool((tk[:, 5] != TOK_FILL).all())))
    s = _base_state(8, 256, 254, 3, 10)
    out.append(("limits_W8_T256", s, lambda p, f, tk, pd: bool((tk != TOK_FILL).all())))
    return out


# ---- shared by tests/test_beam_cpu.py and tests/test_beam_gpu.py ----

STEP_TOL = 1e-4  # per-step log-probability tolerance of the greedy fixture test


def stub_model(E=32, H=4, V=19, layers=2, seed=27, gen_scale=4.0, eos_bias=1.0):
    """Target embedding + decoder + generator of a CSATrans, without the encoder (which has no CPU path): the decoder
    side is all that BeamSearchGenerator.search touches. The generator is sharpened and its EOS logit biased so that
    hypotheses finish at different steps. The default seed and scale were chosen on the CPU oracle alone: among seeds
    1..29 they give the widest decisive gap (0.0101 log-probability at W = 3 and 4) of the runs that show a finished
    hypothesis, a reordering step and a best hypothesis other than greedy's."""
    from csa_amd.glue import LayerNorm
    from csa_amd.model import BaseDecoder, DecoderLayer, Embeddings, Generator
    torch.manual_seed(seed)

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.tgt_embedding = Embeddings(E, V, 0.1, with_pos=True)
            self.decoder = BaseDecoder(DecoderLayer(E, H, 2 * E, 0.2), layers, norm=LayerNorm(E))
            self.generator = Generator(V, E, 0.2)
    m = Stub().eval()
    with torch.no_grad():
        m.generator.linear.weight.mul_(gen_scale)
        m.generator.linear.bias[EOS_ID] += eos_bias
    return m


def search_case(seed=27, B=3, S=7, E=32, device="cpu", **model_kw):
    m = stub_model(E=E, seed=seed, **model_kw).to(device)
    g = torch.Generator().manual_seed(seed + 100)
    enc = torch.randn(B, S, E, generator=g).to(device)
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[1, 4:] = True
    return m, enc, src_mask.to(device)


def assert_oracle_is_decisive(ref, steps):
    """Fails (never skips) unless every decision of the oracle run is wider than twice the accumulated tolerance."""
    assert ref.min_gap > 2 * STEP_TOL * steps, f"smallest decisive gap {ref.min_gap}"


def assert_run_is_interesting(ref, greedy_ids):
    """The oracle run shows a hypothesis finishing before the last step, a step whose parents are not the identity,
    and an AST whose best hypothesis differs from greedy's."""
    W = ref.parents.shape[2]
    assert bool(ref.fin[:-1].any()), "no hypothesis finished before the last step"
    assert bool((ref.parents[1:] != torch.arange(W, device=ref.parents.device)).any()), "parents are always the identity"
    assert bool((ref.best != greedy_ids).any(1).any()), "beam search found what greedy found"


def greedy_ids_ref(m, enc, src_mask, T):
    return beam_search_ref(m, enc, src_mask, T, 1, EOS_ID).best


def run_select(state, device="cpu", t=None):
    """beam_select on tensors built from a hand-built state -> (cum, fin, tokens, pad, anc, parent) as numpy."""
    from csa_amd.decode_ops import beam_select
    ten = {k: torch.from_numpy(np.array(v)).to(device) for k, v in state.items() if isinstance(v, np.ndarray)}
    parent = torch.full((ten["cum"].shape[0],), -1, dtype=torch.int32, device=device)
    t = state["t"] if t is None else t
    beam_select(ten["topv"], ten["topi"], ten["lse"], ten["cum"], ten["fin"], ten["tokens"], ten["pad"], ten["anc"],
                torch.tensor([t], dtype=torch.int32, device=device), eos_id=state["eos_id"], pad_id=PAD,
                parent=parent)
    return tuple(x.cpu().numpy() for x in (ten["cum"], ten["fin"], ten["tokens"], ten["pad"], ten["anc"], parent))


def expected_select(state):
    return select_np(state["topv"], state["topi"], state["lse"], state["cum"], state["fin"], state["tokens"],
                              state["pad"], state["anc"], state["t"], state["eos_id"])


def assert_select_equal(got, want, name):
    for g, w, what in zip(got, want, ("cum", "fin", "tokens", "pad", "anc", "parent")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {what}")
