"""Early stop at EOS on the GPU: k_decode_advance and k_argmax_rows_fin_step (csrc/csa_decode.hip) against numpy, a
parked step of each generator storing nothing, and graph=True + early_stop of the three generators bitwise against eager
+ early_stop and against the full run, with last_steps_run from the rule on the CPU oracles (tests/early_stop_ref.py)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref
import early_stop_ref as ref
import sample_ref
from beam_ref import EOS_ID, PAD, STEP_TOL
from conftest import has_gpu
from early_stop_ref import T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- k_decode_advance ----

def _advance_gpu(fin, t, state, T_, offset):
    from csa_amd.decode_ops import decode_advance
    R = len(fin)
    buf = torch.zeros(R + 1, dtype=torch.uint8, device="cuda")
    f = buf[1:] if offset else buf[:R]  # a base one byte off the allocation's alignment, or on it
    f.copy_(torch.from_numpy(fin))
    t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
    st = torch.tensor(state, dtype=torch.int32, device="cuda")
    decode_advance(f, t_dev, st, T_)
    np.testing.assert_array_equal(f.cpu().numpy(), fin)  # read only
    return int(t_dev.item()), st.tolist()


@pytest.mark.parametrize("R", [1, 3, 64, 255, 256, 257, 1027])
def test_decode_advance_kernel_matches_numpy(R):
    T_ = 9
    rng = np.random.default_rng(R)
    done = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=R)  # any non-zero byte is a finished row
    patterns = [("all", done)]
    for live in sorted({0, R - 1} | ({256} if R > 256 else set())):
        f = done.copy()
        f[live] = 0
        patterns.append((f"live{live}", f))
    for name, fin in patterns:
        for offset in (False, True):
            for all_prev in (0, 1):
                for t in (0, T_ - 2):
                    state = [all_prev, t, 0, 0]
                    got = _advance_gpu(fin, t, state, T_, offset)
                    assert got == ref.advance_np(fin, t, state, T_), (name, offset, all_prev, t)
            state = [1, 4, 1, 0]  # already parked: nothing changes
            assert _advance_gpu(fin, -1, state, T_, offset) == (-1, state), (name, offset)
    # what the cases above must have shown: on with a live row, the latch set without one, parked after it or at the end
    assert ref.advance_np(patterns[1][1], 0, [0, 0, 0, 0], T_) == (1, [0, 1, 0, 0])
    assert ref.advance_np(done, 0, [0, 0, 0, 0], T_) == (1, [1, 1, 0, 0])
    assert ref.advance_np(done, 0, [1, 0, 0, 0], T_) == (-1, [1, 1, 1, 0])
    assert ref.advance_np(patterns[1][1], T_ - 2, [0, T_ - 2, 0, 0], T_) == (-1, [0, T_ - 1, 1, 0])


# ---- k_argmax_rows_fin_step ----

@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("V", [60, 1023, 20000])
def test_argmax_rows_fin_step_kernel_matches_numpy(rows, V):
    from csa_amd.decode_ops import argmax_rows
    T_, H, t = 7, 2, 3
    g = torch.Generator().manual_seed(rows * 31 + V)
    x = torch.randn(rows, V, generator=g)
    # row r: 0 live with an EOS winner, 1 finished with an EOS winner, 2 live with a PAD winner, 3 finished with a
    # random winner, 4 live with a random winner, then the same again
    kind = np.arange(rows) % 5
    for r in range(rows):
        if kind[r] in (0, 1):
            x[r, EOS_ID] = 9.0
        elif kind[r] == 2:
            x[r, PAD] = 9.0
    fin = np.where(np.isin(kind, (1, 3)), np.where(kind == 1, 1, 200), 0).astype(np.uint8)
    tok, padb, fin_after = ref.argmax_fin_np(x.numpy(), fin, EOS_ID)
    assert int(tok[0]) == EOS_ID and int(fin_after[0]) == 1
    ys = torch.full((rows, T_), 9, dtype=torch.long, device="cuda")
    pad = torch.full((rows, T_), 7, dtype=torch.uint8, device="cuda")
    hp = torch.full((rows, H, T_), 7, dtype=torch.uint8, device="cuda")
    keep = [b.clone() for b in (ys, pad, hp)]
    f = torch.from_numpy(fin).cuda()
    xd = x.cuda()
    for bad in (-1, T_ - 1):  # a counter outside its range stores nothing
        argmax_rows(xd, out=ys, is_pad=pad, pad_id=PAD, t_dev=torch.tensor([bad], dtype=torch.int32, device="cuda"),
                    head_pad=hp, fin=f, eos_id=EOS_ID)
        assert _equal([ys, pad, hp], keep) and np.array_equal(f.cpu().numpy(), fin)
    argmax_rows(xd, out=ys, is_pad=pad, pad_id=PAD, t_dev=torch.tensor([t], dtype=torch.int32, device="cuda"),
                head_pad=hp, fin=f, eos_id=EOS_ID)
    np.testing.assert_array_equal(ys[:, t + 1].cpu().numpy(), tok)
    np.testing.assert_array_equal(pad[:, t + 1].cpu().numpy(), padb)
    np.testing.assert_array_equal(f.cpu().numpy(), fin_after)
    np.testing.assert_array_equal(hp.view(H, rows, T_)[:, :, t + 1].cpu().numpy(), np.broadcast_to(padb, (H, rows)))
    other = [c for c in range(T_) if c != t + 1]
    assert torch.equal(ys[:, other], keep[0][:, other]) and torch.equal(pad[:, other], keep[1][:, other])
    assert torch.equal(hp[:, :, other], keep[2][:, :, other])
    ys2, f2 = keep[0].clone(), torch.from_numpy(fin).cuda()  # no mask buffers, no EOS: fin is left alone
    argmax_rows(xd, out=ys2, t_dev=torch.tensor([t], dtype=torch.int32, device="cuda"), fin=f2, eos_id=None)
    np.testing.assert_array_equal(ys2[:, t + 1].cpu().numpy(), tok)
    np.testing.assert_array_equal(f2.cpu().numpy(), fin)


# ---- the generators ----

_CASES, _ORACLES = {}, {}


def _case(name, mem_seed=None):
    """(model, enc, src_mask) of a named case on the GPU: one model per name, built once and never modified, so that
    two memories go through one captured graph."""
    if name not in _CASES:
        _CASES[name] = ref.tiny_model(**getattr(ref, name)).cuda()
    return (_CASES[name], *ref.tiny_memory(getattr(ref, name)["seed"] if mem_seed is None else mem_seed, "cuda"))


def _oracle(kind, mem_seed=None):
    """The CPU oracle of a generator's case run for all steps, and steps_run by the rule; computed once."""
    if (kind, mem_seed) not in _ORACLES:
        if kind == "beam":
            m, enc, src_mask = ref.tiny_case(ref.BEAM_STOPS, mem_seed)
            r = beam_ref.beam_search_ref(m, enc, src_mask, T, 4, EOS_ID)
            beam_ref.assert_oracle_is_decisive(r, T - 1)
            fins = r.fin.reshape(T - 1, -1).numpy()
        elif kind == "sampling":
            m, enc, src_mask = ref.tiny_case(ref.NEVER, mem_seed)
            r = sample_ref.sampling_ref(m, enc, src_mask, T, 4, ref.SAMPLING_SEED, **ref.SAMPLING)
            sample_ref.assert_decisive(r)
            fins = r.fin
        else:
            m, enc, src_mask = ref.tiny_case(ref.GREEDY, mem_seed)
            ids, fins, gap = ref.greedy_eos_ref(m, enc, src_mask, T, EOS_ID)
            assert gap > ref.GREEDY_GAP
            r, fins = SimpleNamespace(ids=ids), fins.numpy()
        _ORACLES[kind, mem_seed] = (r, ref.steps_rule(fins, T - 1))
    return _ORACLES[kind, mem_seed]


_NAME = {"greedy": "GREEDY", "beam": "BEAM_STOPS", "sampling": "NEVER"}


def _make(kind, **kw):
    """-> (generator, run): run(mem_seed=None) makes one call on that memory and returns its outputs as a tuple."""
    from csa_amd.model import BeamSearchGenerator, CachedGreedyGenerator, SamplingGenerator
    m = _case(_NAME[kind])[0]
    if kind == "beam":
        gen = BeamSearchGenerator(m, T, 4, **kw)
        return gen, lambda mem_seed=None: gen.search(*_case("BEAM_STOPS", mem_seed)[1:], return_all=True)
    if kind == "sampling":
        gen = SamplingGenerator(m, T, num_samples=4, **ref.SAMPLING, **kw)
        return gen, lambda mem_seed=None: gen.sample(*_case("NEVER", mem_seed)[1:], seed=ref.SAMPLING_SEED,
                                                     return_logp=True)
    fixed = ref.FixedMemory(m, None, None)
    gen = CachedGreedyGenerator(fixed, T, eos_id=EOS_ID, **kw)

    def run(mem_seed=None):
        fixed.enc, fixed.src_mask = _case("GREEDY", mem_seed)[1:]
        return gen(SimpleNamespace(), return_logp=True)
    return gen, run


def _check_against_oracle(kind, out, want):
    if kind == "beam":
        assert torch.equal(out[1].cpu(), want.ids) and torch.equal(out[0].cpu(), want.best)
        np.testing.assert_allclose(out[2].cpu().numpy(), want.scores.numpy(), rtol=0, atol=STEP_TOL * (T - 1))
    elif kind == "sampling":
        assert torch.equal(out[0].cpu(), want.ids)
        np.testing.assert_allclose(out[1].cpu().numpy(), want.logp, rtol=sample_ref.RTOL, atol=sample_ref.ATOL)
    else:
        assert torch.equal(out[0].cpu(), want.ids)


OTHER_MEMORY = 77  # a second memory, whose batch finishes at another step (asserted on the oracles)


@pytest.mark.parametrize("kind", ["greedy", "beam", "sampling"])
def test_graph_early_stop_is_bitwise_eager_and_the_full_run(kind):
    want, steps = _oracle(kind)
    want2, steps2 = _oracle(kind, OTHER_MEMORY)
    assert steps < T - 1 and steps2 < T - 1 and steps != steps2
    full, run_full = _make(kind)
    eager, run_eager = _make(kind, early_stop=True)
    gen, run = _make(kind, early_stop=True, graph=True)
    a, b, c = run_full(), run_eager(), run()
    print(kind, "steps_run", gen.last_steps_run, "replays", gen.last_replays, "of", T - 1)
    _check_against_oracle(kind, c, want)
    if kind == "greedy":  # the log-probabilities of the steps that ran
        assert a[1].shape[0] == T - 1 and b[1].shape[0] == steps and c[1].shape[0] == steps
        a = (a[0], a[1][:steps])
    assert _equal(a, b) and _equal(b, c)
    assert full.last_steps_run == T - 1 and eager.last_steps_run == steps and eager.last_replays == steps
    assert gen.last_steps_run == steps and gen.last_replays <= steps + 2 * gen.poll_every
    assert _equal(run(), c) and gen.captures == 1 and eager.captures == 0  # two calls capture once
    # a second batch through the same graph finishes at another step: the latch, fin and the counter are reset
    c2 = run(OTHER_MEMORY)
    assert gen.captures == 1 and gen.last_steps_run == steps2
    _check_against_oracle(kind, c2, want2)
    assert _equal(run_eager(OTHER_MEMORY), c2) and eager.last_steps_run == steps2
    assert _equal(run(), c) and gen.last_steps_run == steps  # and back again
    for poll in (1, 3, 8):
        gen.poll_every = poll
        assert _equal(run(), c), poll
        assert gen.last_steps_run == steps and steps <= gen.last_replays <= min(T - 1, steps + 2 * poll), poll
    assert gen.captures == 1
    # early_stop=False keeps its own graph key: a generator without the keyword captures the plain step
    plain, run_plain = _make(kind, graph=True)
    assert _equal(run_plain(), run_full()) and plain.last_steps_run == T - 1 and plain.last_replays == T - 1


def _graph_nodes(gen):
    (entry,) = gen._graphs.values()
    with open("/proc/self/maps") as f:  # the HIP runtime torch has loaded, not a second copy of it
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    n = ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(ctypes.c_void_p(entry.graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return int(n.value)


@pytest.mark.parametrize("kind", ["greedy", "beam", "sampling"])
def test_the_latch_replaces_the_increment_node_for_node(kind):
    """The captured step with early_stop has as many nodes as without it (csa_decode_advance stands where the
    counter's increment stood), and for greedy eos_id alone adds none either (one argmax kernel for the other)."""
    nodes = {}
    for name, kw in (("plain", {}), ("early", dict(early_stop=True))):
        gen, run = _make(kind, graph=True, **kw)
        gen._keep_graph = True
        run()
        assert gen.captures == 1
        nodes[name] = _graph_nodes(gen)
    if kind == "greedy":
        from csa_amd.model import CachedGreedyGenerator
        m, enc, src_mask = _case("GREEDY")
        gen = CachedGreedyGenerator(ref.FixedMemory(m, enc, src_mask), T, graph=True)  # no eos_id: today's step
        gen._keep_graph = True
        gen(SimpleNamespace(), return_logp=True)  # as _make's calls: the log-softmax is a node of the step
        nodes["no_eos"] = _graph_nodes(gen)
        assert gen.last_steps_run == T - 1 and nodes["no_eos"] == nodes["plain"]
    print(kind, "captured nodes:", nodes)
    assert nodes["early"] == nodes["plain"]


@pytest.mark.parametrize("kind", ["greedy", "beam", "sampling"])
def test_a_parked_step_stores_nothing(kind):
    gen, _ = _make(kind, early_stop=True)
    m, enc, src_mask = _case(_NAME[kind])
    with torch.no_grad():
        cache = m.decoder.make_cache(enc, src_mask, T, **gen._cache_options)
        e = gen._state(cache, return_logp=kind == "sampling")
        gen._reset(e)
        if kind == "sampling":
            e.rng.copy_(torch.tensor([ref.SAMPLING_SEED, 0]))
        for _ in range(2):  # two real steps, so that the buffers hold something
            gen._device_step(e)
        assert int(e.t_dev.item()) == 2 and e.stop.tolist()[1:3] == [2, 0]
        e.t_dev.fill_(-1)
        e.stop.copy_(torch.tensor([1, 2, 1, 0], dtype=torch.int32))
        bufs = {"ys": e.ys, "pad": cache.pad, "fin": e.fin, "t_dev": e.t_dev, "stop": e.stop}
        for k, v in (("head_pad", cache.head_pad), ("anc", cache.anc), ("cum", getattr(e, "cum", None)),
                     ("logp", e.logp if kind == "sampling" else None)):
            if v is not None:
                bufs[k] = v
        for i in range(len(cache.self_k)):
            bufs[f"k{i}"], bufs[f"v{i}"], bufs[f"mem{i}"] = cache.self_k[i], cache.self_v[i], cache.memory_kv[i]
        assert {"greedy": "head_pad", "beam": "anc", "sampling": "logp"}[kind] in bufs
        before = {k: v.clone() for k, v in bufs.items()}
        gen._device_step(e)
        torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v.view(torch.uint8) if v.is_floating_point() else v,
                           before[k].view(torch.uint8) if v.is_floating_point() else before[k]), k
    assert int(e.t_dev.item()) == -1


# the production-dim decoder of test_beam_gpu.PROD_BEAM with a larger EOS bias, chosen on the CPU oracle alone (biases 1,
# 3, 5, 7): the first with which every hypothesis finishes early (after step 2 of 9); smallest decisive gap 0.0334
PROD = dict(seed=5, gen_scale=4.0, eos_bias=3.0)


def test_early_stop_at_production_head_dim():
    """hd = 64, S = 150, E = 512, two layers, padded source: the captured early-stopping beam against the oracle and,
    bitwise, against the full run."""
    from csa_amd.model import BeamSearchGenerator
    T_, W, B, S, E = 10, 3, 2, 150, 512
    m, enc, _ = beam_ref.search_case(B=B, S=S, E=E, H=8, V=120, **PROD)
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[0, 120:] = True
    src_mask[1, 37:] = True
    want = beam_ref.beam_search_ref(m, enc, src_mask, T_, W, EOS_ID)
    beam_ref.assert_oracle_is_decisive(want, T_ - 1)
    steps = ref.steps_rule(want.fin.reshape(T_ - 1, -1).numpy(), T_ - 1)
    assert steps < T_ - 1
    m, enc, src_mask = m.cuda(), enc.cuda(), src_mask.cuda()
    full = BeamSearchGenerator(m, T_, W)
    gen = BeamSearchGenerator(m, T_, W, graph=True, early_stop=True)
    a, b = full.search(enc, src_mask, return_all=True), gen.search(enc, src_mask, return_all=True)
    print(f"steps_run {gen.last_steps_run} of {T_ - 1}, replays {gen.last_replays}, min_gap={want.min_gap:.6f}")
    assert torch.equal(b[1].cpu(), want.ids) and torch.equal(b[0].cpu(), want.best)
    np.testing.assert_allclose(b[2].cpu().numpy(), want.scores.numpy(), rtol=0, atol=STEP_TOL * (T_ - 1))
    assert _equal(a, b) and gen.last_steps_run == steps and gen.last_replays <= steps + 2 * gen.poll_every
