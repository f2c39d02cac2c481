"""Scoring given summaries on the GPU: k_token_logp_* (csrc/csa_score.hip) through the C ABI and the op in every launch
class against the fp64 oracle, SequenceScorer against the reference's fixtures, against what SamplingGenerator and
BeamSearchGenerator accumulated for the same ids, and under autograd (tests/score_ref.py)."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import score_ref
from conftest import has_gpu
from golden_inputs import fill_params_deterministic
from score_ref import ATOL, EOS_ID, PAD, RTOL, TINY, assert_same_kind_and_close

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

# the forward's launch classes (include/csa_hip.h): register-resident rows up to 4096 NG columns, NG = 1..6, streaming
# above 24576; each threshold at -1, 0 and +1, the smallest rows, an odd size and the 50021-word vocabulary
THRESHOLDS = [4096 * ng for ng in range(1, 7)]
VS = [1, 2, 3, 1003] + [th + d for th in THRESHOLDS for d in (-1, 0, 1)] + [50021]
ROWS = [1, 5, 33]
SENTINEL = 777.0


@functools.lru_cache(maxsize=None)
def class_case(V):
    """Inputs and fp64 results of a launch class for the largest row count, computed once and never modified: a row
    depends on its own logits alone, so the smaller launches are its first rows."""
    ig = score_ref.kernel_ignore_id(V)
    z, t, g = score_ref.kernel_case(max(ROWS), V)
    return z, t, g, ig, score_ref.token_logp_ref(z, t, ig), score_ref.token_logp_grad_ref(z, t, g, ig)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _layouts(z):
    """(name, (rows, V) CUDA view of z's values, its row stride): contiguous; a wider buffer (ld > V, so the rows' base
    alignments differ); a base address that is 4-byte but not 16-byte aligned."""
    rows, V = z.shape
    out = [("contiguous", z.cuda(), V)]
    wide = torch.full((rows, V + 3), SENTINEL, device="cuda")
    wide[:, :V] = z.cuda()
    out.append(("ld_gt_V", wide[:, :V], V + 3))
    flat = torch.full((rows * V + 4,), SENTINEL, device="cuda")
    flat[1:1 + rows * V] = z.cuda().reshape(-1)
    out.append(("base_plus_4_bytes", flat[1:1 + rows * V].view(rows, V), V))
    return out


def _abi(zv, ld, t, g, ig):
    """Forward, backward and in-place backward through the C ABI on the view zv -> (logp, lse, dz, dz in place)."""
    from csa_amd._lib import check, lib
    L = lib()
    rows, V = zv.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    logp = torch.full((rows,), SENTINEL, device="cuda")
    lse = torch.full((rows, 2), SENTINEL, device="cuda")
    check(L.csa_token_logp_fwd(_p(zv), ld, _p(t), rows, V, ig, _p(logp), _p(lse), st), "fwd")
    dz = torch.full((rows, V + 1), SENTINEL, device="cuda")
    check(L.csa_token_logp_bwd(_p(g), _p(zv), ld, _p(t), _p(lse), _p(dz), V + 1, rows, V, ig, st), "bwd")
    assert bool((dz[:, V] == SENTINEL).all())  # nothing beyond a row's V columns is written
    # in place on a copy with the same layout (same base alignment, same ld)
    off = (zv.data_ptr() % 16) // 4
    buf = torch.full((rows * ld + 4,), SENTINEL, device="cuda")
    inplace = buf[off:off + rows * ld].view(rows, ld)[:, :V]
    assert inplace.data_ptr() % 16 == zv.data_ptr() % 16
    inplace.copy_(zv)
    check(L.csa_token_logp_bwd(_p(g), _p(inplace), ld, _p(t), _p(lse), _p(inplace), ld, rows, V, ig, st), "bwd in place")
    return logp, lse, dz[:, :V], inplace


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_token_logp_kernels_match_fp64_in_every_launch_class(V, rows):
    from csa_amd.score_ops import token_logp
    z, t, g, ig, want, want_dz = class_case(V)
    # a launch of one row is run once per row kind (the kinds are the first rows of the class's case)
    picks = [slice(i, i + 1) for i in range(len(score_ref.KINDS))] if rows == 1 else [slice(0, rows)]
    for pick in picks:
        zc, tc, gc = z[pick], t[pick].cuda(), g[pick].cuda()
        first = None
        for name, zv, ld in _layouts(zc):
            what = f"V={V} rows={rows} first={pick.start} {name}"
            logp, lse, dz, inplace = _abi(zv, ld, tc, gc, ig)
            assert_same_kind_and_close(logp, want[pick], what + " logp")
            assert_same_kind_and_close(dz, want_dz[pick], what + " dz")
            assert torch.equal(dz.contiguous().view(torch.int32), inplace.contiguous().view(torch.int32)), what  # bitwise
            ignored = ~score_ref.scored_rows(t[pick], V, ig)
            assert bool((logp[ignored.cuda()] == 0).all()) and bool((dz[ignored.cuda()] == 0).all()), what
            assert not bool((lse == SENTINEL).any()), what  # lse is written for every row, ignored ones included
            # the op: the same launches on the same view, and autograd's gradient of the leaf behind the view
            leaf = zv.detach().clone().requires_grad_() if name == "contiguous" else None
            out = token_logp(leaf if leaf is not None else zv, tc, ignore_id=ig)
            assert torch.equal(out.view(torch.int32), logp.view(torch.int32)), what
            if leaf is not None:
                out.backward(gc)
                assert torch.equal(leaf.grad.view(torch.int32), dz.contiguous().view(torch.int32)), what
            # the summation order belongs to the class, not to the layout, but vector and scalar loads take the same
            # columns per lane: every layout gives the same bits
            if first is None:
                first = (logp, dz.contiguous())
            else:
                assert torch.equal(first[0].view(torch.int32), logp.view(torch.int32)), what
                assert torch.equal(first[1].view(torch.int32), dz.contiguous().view(torch.int32)), what


def test_token_logp_op_takes_views_shapes_and_the_fallbacks():
    from csa_amd.score_ops import token_logp, token_logp_host
    z, t, g, ig, want, _ = class_case(1003)
    zc, tc = z[:24].cuda(), t[:24].cuda()
    out = token_logp(zc.view(2, 3, 4, 1003), tc.view(2, 3, 4), ignore_id=ig)
    assert out.shape == (2, 3, 4) and out.dtype == torch.float32
    assert_same_kind_and_close(out.view(-1), want[:24], "4-d logits")
    assert_same_kind_and_close(token_logp(zc.t().contiguous().t(), tc, ignore_id=ig), want[:24], "strided last dim")
    assert_same_kind_and_close(token_logp_host(zc, tc, ig), want[:24], "fallback on the device")
    assert_same_kind_and_close(token_logp(zc.double(), tc, ignore_id=ig), want[:24], "fp64 logits", rtol=1e-10, atol=1e-12)
    assert token_logp(zc[:0], tc[:0]).shape == (0,)


# ---- the reference's fixtures ----

def _tiny(seed, gen_scale=1.0, eos_bias=0.0):
    from csa_amd.model import CSATrans
    m = CSATrans(**TINY)
    fill_params_deterministic(m, seed)
    with torch.no_grad():
        m.generator.linear.weight.mul_(gen_scale)
        m.generator.linear.bias[EOS_ID] += eos_bias
    return m.cuda().eval()


def _arm(m, z):
    """The fixture's STE uniforms for the next encode (the attention consumes them)."""
    for i in range(2):
        getattr(m.SBM, f"transformer_{i}").mha.attn.uniforms = torch.from_numpy(z[f"u{i}"]).cuda()


def test_scorer_reproduces_the_training_forward_of_the_reference(golden):
    """tests/golden/csatrans_tiny.npz, built as test_csatrans_forward_backward_matches_reference builds it: the
    scorer's per-token log-probabilities are the reference's `out` gathered at the target, and validation_nll is its
    loss."""
    from csa_amd.model import SequenceScorer, batch_to_device, validation_nll
    z = golden("csatrans_tiny")
    assert np.array_equal(z["tgt_seq"][:, 1:], z["target"][:, :-1]) and (z["tgt_seq"][:, 0] == score_ref.BOS).all()
    m = _tiny(71)
    keys = ("src_seq", "tgt_seq", "target", "L", "T", "L_mask", "T_mask")
    x, y = batch_to_device({k: z[k] for k in keys}, torch.device("cuda"))
    _arm(m, z)
    with torch.no_grad():
        out = SequenceScorer(m, head_mask="reference")(x, y, return_tokens=True)
    want = np.take_along_axis(z["out"], z["target"][:, :, None], 2)[:, :, 0]
    assert np.isfinite(want).all()
    scored = score_ref.scored_positions(torch.from_numpy(z["target"]), EOS_ID).numpy()
    assert np.array_equal(scored, z["target"] != PAD)
    np.testing.assert_allclose(out.tokens.cpu().numpy(), np.where(scored, want, 0.0), rtol=1e-4, atol=1e-4)
    assert out.length.tolist() == scored.sum(1).tolist()
    x, y = batch_to_device({k: z[k] for k in keys}, torch.device("cuda"))
    _arm(m, z)
    nll = validation_nll(m, [(x, y)])
    assert nll.tokens == int(scored.sum())
    np.testing.assert_allclose(nll.nll, z["loss"][0], rtol=1e-5)
    np.testing.assert_allclose(nll.ppl, np.exp(np.float64(z["loss"][0])), rtol=1e-4)


def test_scorer_reproduces_the_greedy_fixture_of_the_reference(golden):
    """tests/golden/greedy_tiny.npz: scoring the reference's greedy ids with its own head mask and no EOS rule gives
    its per-step log-probabilities at those ids."""
    from csa_amd.model import SequenceScorer
    z = golden("greedy_tiny")
    seed, _ = (int(v) for v in z["meta"])
    m = _tiny(seed, 8.0)
    _arm(m, z)
    c = lambda k, dt: torch.from_numpy(z[k]).to(dt).cuda()
    data = SimpleNamespace(src_seq=c("src_seq", torch.int64), tgt_seq=None, L=c("L", torch.uint8), T=c("T", torch.uint8),
                           L_mask=c("L_mask", torch.uint8), T_mask=c("T_mask", torch.uint8))
    ys = c("ys", torch.int64)
    with torch.no_grad():
        out = SequenceScorer(m, eos_id=None, head_mask="reference")(data, ys, return_tokens=True)
    want = np.take_along_axis(z["step_logp"].transpose(1, 0, 2), z["ys"][:, :, None], 2)[:, :, 0]
    np.testing.assert_allclose(out.tokens.cpu().numpy(), want, rtol=1e-4, atol=1e-4)
    assert out.length.tolist() == [z["ys"].shape[1]] * z["ys"].shape[0]


# ---- against the generators ----

T_GEN = 8


@functools.lru_cache(maxsize=None)
def _generator_case():
    """The tiny model (its generator sharpened and its EOS biased so that rows finish at different steps), a batch of
    three synthetic ASTs and their encoder output, computed once on the GPU."""
    from csa_amd.data import synthetic_batch
    from csa_amd.model import batch_to_device
    m = _tiny(6, 8.0, 2.0)
    sb = synthetic_batch(3, max_size=20, seed=4, min_nodes=12, max_nodes=20, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
    data, _ = batch_to_device(sb, torch.device("cuda"))
    torch.manual_seed(3)
    with torch.no_grad():
        m.process_data(data)
        enc = m.encode(data)[0]
    return m, enc, data.src_mask


def _oracle(m, enc, src_mask, ids):
    return score_ref.score_loop_ref(m, enc, src_mask, ids.cpu(), EOS_ID, "own")


def test_scorer_equals_the_samplers_log_probabilities():
    from csa_amd.model import SamplingGenerator, SequenceScorer
    m, enc, src_mask = _generator_case()
    gen = SamplingGenerator(m, T_GEN, temperature=1.0, top_k=0, top_p=1.0, num_samples=2)
    ids, lp = gen.sample(enc, src_mask, seed=17, return_logp=True)
    with torch.no_grad():
        out = SequenceScorer(m).score(enc, src_mask, ids, return_tokens=True)
    tokens, logp, length = _oracle(m, enc, src_mask, ids)
    R = ids.shape[0] * ids.shape[1]
    print("sampler vs fp64", (lp.view(R, -1).cpu().double() - tokens).abs().max().item(),
          "scorer vs fp64", (out.tokens.view(R, -1).cpu().double() - tokens).abs().max().item())
    np.testing.assert_allclose(lp.view(R, -1).cpu().numpy(), tokens.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.tokens.view(R, -1).cpu().numpy(), tokens.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.tokens.cpu().numpy(), lp.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)
    assert out.length.view(-1).tolist() == length.tolist()


def test_scorer_equals_the_beams_scores_and_keeps_its_order():
    from csa_amd.model import BeamSearchGenerator, SequenceScorer, rerank
    m, enc, src_mask = _generator_case()
    W = 3
    best, ids, scores = BeamSearchGenerator(m, T_GEN, W, length_penalty=0.0).search(enc, src_mask, return_all=True)
    with torch.no_grad():
        out = SequenceScorer(m).score(enc, src_mask, ids)
    _, logp, _ = _oracle(m, enc, src_mask, ids)
    print("beam vs fp64", (scores.view(-1).cpu().double() - logp).abs().max().item(),
          "scorer vs fp64", (out.logp.view(-1).cpu().double() - logp).abs().max().item())
    np.testing.assert_allclose(scores.view(-1).cpu().numpy(), logp.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.view(-1).cpu().numpy(), logp.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.cpu().numpy(), scores.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)
    top, order = rerank(ids, out, length_penalty=0.0)
    assert order.tolist() == [list(range(W))] * ids.shape[0]
    assert torch.equal(top, best)


# ---- autograd ----

def test_scorer_gradients_match_the_log_softmax_chain():
    """out.logp.sum().backward() through the scorer against the same loss built from torch.log_softmax + gather on the
    same modules; through forward() the gradient also reaches the encoder."""
    from csa_amd.data import synthetic_batch
    from csa_amd.model import SequenceScorer, batch_to_device, make_std_mask
    m, enc, src_mask = _generator_case()
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(4, 60, (3, 2, T_GEN - 1), generator=g)
    ids[0, 0, 3], ids[1, 1, 5], ids[2, 0, 1] = EOS_ID, EOS_ID, EOS_ID
    ids = ids.cuda()
    params = {k: p for k, p in m.named_parameters() if k.startswith(("decoder.", "generator.", "tgt_embedding."))}

    def grads(loss_fn):
        m.zero_grad(set_to_none=True)
        e = enc.clone().requires_grad_()
        loss_fn(e).backward()
        out = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
        out["enc"] = e.grad.detach().clone()
        return out

    scorer = SequenceScorer(m)

    def chain(e):
        R = 6
        cand = ids.view(R, -1)
        dec_in = torch.cat([torch.full((R, 1), score_ref.BOS, device="cuda"), cand[:, :-1]], 1)
        mask = make_std_mask(dec_in, PAD).repeat_interleave(8, 0)
        dec, _ = m.decoder(m.tgt_embedding(dec_in).permute(1, 0, 2), e.repeat_interleave(2, 0).permute(1, 0, 2),
                           tgt_mask=mask, memory_key_padding_mask=src_mask.repeat_interleave(2, 0))
        lp = torch.log_softmax(m.generator.linear(dec.permute(1, 0, 2)), -1).gather(2, cand[:, :, None])[:, :, 0]
        scored = score_ref.scored_positions(cand.cpu(), EOS_ID).cuda()
        return torch.where(scored, lp, torch.zeros_like(lp)).sum()

    try:
        got = grads(lambda e: scorer.score(e, src_mask, ids).logp.sum())
        want = grads(chain)
        assert got.keys() == want.keys() and len(got) > 40
        assert any(k.startswith("generator.") for k in got) and any(k.startswith("decoder.") for k in got)
        for k in want:
            np.testing.assert_allclose(got[k].cpu().numpy(), want[k].cpu().numpy(), rtol=1e-3, atol=2e-5, err_msg=k)
        # forward(): process_data + encode under autograd, so an encoder parameter gets a gradient too
        m.zero_grad(set_to_none=True)
        sb = synthetic_batch(3, max_size=20, seed=4, min_nodes=12, max_nodes=20, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
        data, _ = batch_to_device(sb, torch.device("cuda"))
        scorer(data, ids).logp.sum().backward()
        w = m.SBM.out.weight.grad
        assert w is not None and bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
        assert m.generator.linear.weight.grad is not None
    finally:
        m.zero_grad(set_to_none=True)


def test_token_logp_peak_memory_is_below_the_log_softmax_chain():
    """Forward + backward at (rows, V) = (512, 50021): the op saves 8 bytes per row and writes one (rows, V) gradient;
    log_softmax + gather saves a (rows, V) output and builds the gradient from it."""
    from csa_amd.score_ops import token_logp
    rows, V = 512, 50021
    gen = torch.Generator().manual_seed(2)
    z = torch.randn(rows, V, generator=gen).cuda()
    t = torch.randint(1, V, (rows,), generator=gen).cuda()

    def peak(fn):
        zz = z.clone().requires_grad_()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(zz).sum().backward()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        return p, zz.grad

    p_op, g_op = peak(lambda zz: token_logp(zz, t))
    p_chain, g_chain = peak(lambda zz: torch.log_softmax(zz, -1).gather(1, t[:, None])[:, 0])
    print(f"peak bytes above the inputs: token_logp {p_op}, log_softmax + gather {p_chain}")
    np.testing.assert_allclose(g_op[:4].cpu().numpy(), g_chain[:4].cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert p_op < p_chain
