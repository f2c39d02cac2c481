"""What scoring given summaries costs at the config/java.py dims: 64 ASTs of 150 nodes, candidates of 49 tokens
(max_tgt_len 50), G = 1 and G = 4 candidates per AST, eval mode, no_grad, from a precomputed encoder output. Two legs:

  generator  what a user could do before: the teacher-forced decoder pass, model.generator(dec) (the (rows, V)
             log(softmax) tensor), gather at the candidates, mask after the first EOS, sum
  scorer     SequenceScorer.score: the same pass, generator.linear, score_ops.token_logp

and the op alone at the same (rows, V): token_logp against torch.log_softmax(...).gather(...), forward and
forward + backward, between HIP events, with torch.cuda.max_memory_allocated above the inputs for each.

With --fused, the legs of the fused full-sequence decoder attention instead (profiles/seq_score_fused.json):

  sdpa / fused   SequenceScorer(attention=...) at G = 1 and 4, forward under no_grad and forward + backward of
                 logp.sum() to the decoder, the generator and the encoder output, with the peak memory of each
  seq_attention  the op alone against F.scaled_dot_product_attention with the explicit -inf masks and expanded K/V
                 (seq_attn_ops.seq_attention_sdpa), at the cross-attention shape (R = batch * G, T, S = nodes,
                 kv_group = G, a memory mask) and the self-attention shape (causal, a row's own PAD columns), forward
                 and forward + backward between HIP events

usage: python tools/bench_score.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--calls 3] [--reps 5]
                                   [--out profiles/seq_score.json] [--fused [--fused-out profiles/seq_score_fused.json]]

Both legs live in one process on one GPU and are timed alternately: per rep, every leg runs `calls` scoring calls
between two device synchronisations on the host clock. The JSON keeps the median of the reps, every rep and the
max - min spread per leg, and says whether the legs are resolved from each other by more than their spreads. Nothing is
compared against a promise: the numbers are what they are. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import torch  # noqa: E402

LEGS = ("generator", "scorer")
GROUPS = (1, 4)


def events_ms(fn, reps):
    """All of `reps` HIP-event timings of fn() after one warm-up call."""
    fn()
    out = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return out


def peak_bytes(fn):
    """torch.cuda.max_memory_allocated of one fn() call above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def summary(ms):
    return {"median": statistics.median(ms), "all": ms, "spread": max(ms) - min(ms)}


def resolved(a, b):
    return abs(a["median"] - b["median"]) > max(a["spread"], b["spread"])


def fused_legs(a, model, enc, src_mask, cands, res):
    """The --fused legs (module docstring) into res["groups"] and res["op"]."""
    from csa_amd.data import EOS
    from csa_amd.model import PAD, SequenceScorer
    from csa_amd.seq_attn_ops import seq_attention, seq_attention_sdpa
    legs = ("sdpa", "fused")
    scorers = {leg: SequenceScorer(model, eos_id=EOS, head_mask="own", attention=leg) for leg in legs}
    H = model.decoder.layers[0].self_attn.num_heads
    hd = enc.shape[-1] // H
    dev = enc.device
    for G, cand in cands.items():
        def fwd(leg):
            with torch.no_grad():
                return scorers[leg].score(enc, src_mask, cand).logp

        def fwd_bwd(leg):
            model.zero_grad(set_to_none=True)
            e = enc.detach().requires_grad_()
            scorers[leg].score(e, src_mask, cand).logp.sum().backward()
            return e.grad

        def run(fn, leg, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn(leg)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        out = {"max_abs_difference_of_scores": float((fwd("sdpa") - fwd("fused")).abs().max()),
               "max_abs_difference_of_enc_grad": float((fwd_bwd("sdpa") - fwd_bwd("fused")).abs().max()),
               "last_attention": scorers["fused"].last_attention, "rows": cand.shape[0] * G * cand.shape[2]}
        for key, fn in (("fwd_ms", fwd), ("fwd_bwd_ms", fwd_bwd)):
            for leg in legs:
                run(fn, leg, 2)
            ms = {leg: [] for leg in legs}
            for _ in range(a.reps):
                for leg in legs:
                    ms[leg].append(run(fn, leg, a.calls))
            out[key] = {leg: summary(ms[leg]) for leg in legs}
            for leg in legs:
                out[key][leg]["peak_bytes"] = peak_bytes(lambda: fn(leg))
            out[key]["fused_minus_sdpa_ms"] = out[key]["fused"]["median"] - out[key]["sdpa"]["median"]
            out[key]["resolved"] = resolved(out[key]["fused"], out[key]["sdpa"])
        model.zero_grad(set_to_none=True)
        res["groups"][f"G={G}"] = out

        # the op alone: the cross-attention and the self-attention of one layer at this G
        R, T, S = a.batch * G, cand.shape[2], enc.shape[1]
        pad = (cand.reshape(R, T) == PAD).to(torch.uint8)
        pad[:, 0] = 0  # the decoder input starts with BOS
        shapes = {"cross": dict(k_rows=a.batch, S=S, key_mask=src_mask.to(torch.uint8), causal=False, kv_group=G),
                  "self": dict(k_rows=R, S=T, key_mask=pad, causal=True, kv_group=1)}
        op_out = {}
        for name, sh in shapes.items():
            q = torch.randn(R, H, T, hd, device=dev)
            k, v = (torch.randn(sh["k_rows"], H, sh["S"], hd, device=dev) for _ in range(2))
            g = torch.randn(R, T, H * hd, device=dev)
            kw = dict(key_mask=sh["key_mask"], causal=sh["causal"], mask_mode="own", kv_group=sh["kv_group"])
            ops = {"seq_attention": lambda *t: seq_attention(*t, **kw), "sdpa": lambda *t: seq_attention_sdpa(*t, **kw)}
            leaves = [t.clone().requires_grad_() for t in (q, k, v)]

            def op_fwd(fn):
                with torch.no_grad():
                    return fn(q, k, v)

            def op_fwd_bwd(fn):
                for t in leaves:
                    t.grad = None
                fn(*leaves).backward(g)

            timed = {(n, key): (lambda fn=fn, f=f: f(fn)) for n, fn in ops.items()
                     for key, f in (("fwd_ms", op_fwd), ("fwd_bwd_ms", op_fwd_bwd))}
            op_ms = {key: [] for key in timed}
            for fn in timed.values():
                fn()
            for _ in range(a.reps):
                for key, fn in timed.items():
                    op_ms[key] += events_ms(fn, 1)
            o = {n: {key: summary(op_ms[n, key]) for key in ("fwd_ms", "fwd_bwd_ms")} for n in ops}
            for n, fn in ops.items():
                o[n]["fwd_peak_bytes"] = peak_bytes(lambda: op_fwd(fn))
                o[n]["fwd_bwd_peak_bytes"] = peak_bytes(lambda: op_fwd_bwd(fn))
            for t in leaves:
                t.grad = None
            for key in ("fwd_ms", "fwd_bwd_ms"):
                o[key + "_resolved"] = resolved(o["seq_attention"][key], o["sdpa"][key])
            o["max_abs_difference"] = float((op_fwd(ops["seq_attention"]) - op_fwd(ops["sdpa"])).abs().max())
            o["shape"] = {"R": R, "H": H, "T": T, "S": sh["S"], "hd": hd, "kv_group": sh["kv_group"]}
            op_out[name] = o
        res["op"][f"G={G}"] = op_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=150)
    ap.add_argument("--max-tgt-len", type=int, default=50)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_score.json"))
    ap.add_argument("--fused", action="store_true", help="the legs of the fused full-sequence decoder attention")
    ap.add_argument("--fused-out", default=os.path.join(ROOT, "profiles", "seq_score_fused.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import BOS, EOS, synthetic_batch
    from csa_amd.model import CONFIGS, PAD, CSATrans, SequenceScorer, batch_to_device, make_std_mask
    from csa_amd.score_ops import token_logp

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    cfg = CONFIGS["java"]
    V, H = cfg["tgt_vocab_size"], cfg["num_heads"]
    model = CSATrans(**cfg).to(dev).eval()
    data, _ = batch_to_device(synthetic_batch(a.batch, max_size=a.nodes, seed=a.seed, max_tgt_len=a.max_tgt_len), dev)
    with torch.no_grad():
        model.process_data(data)
        enc = model.encode(data)[0]
    src_mask = data.src_mask
    T = a.max_tgt_len - 1
    scorer = SequenceScorer(model, eos_id=EOS, head_mask="own")

    def generator_leg(cand):
        """The route through model.generator: the scorer's pass with the (rows, V) log-probabilities materialised."""
        B, G, _ = cand.shape
        c = cand.reshape(B * G, T)
        dec_in = torch.cat([torch.full((B * G, 1), BOS, dtype=torch.int64, device=dev), c[:, :-1]], 1)
        mask = make_std_mask(dec_in, PAD).repeat_interleave(H, 0)
        dec, _ = model.decoder(model.tgt_embedding(dec_in).permute(1, 0, 2),
                               enc.repeat_interleave(G, 0).permute(1, 0, 2), tgt_mask=mask,
                               memory_key_padding_mask=src_mask.repeat_interleave(G, 0))
        logp = model.generator(dec.permute(1, 0, 2)).gather(2, c[:, :, None])[:, :, 0]
        is_eos = (c == EOS).to(torch.int32)
        scored = (is_eos.cumsum(1) - is_eos) == 0
        return torch.where(scored, logp, torch.zeros_like(logp)).sum(-1).view(B, G)

    res = {
        "what": "teacher-forced scoring of G candidates per AST from a precomputed encoder output, eval mode, no_grad: "
                "model.generator(dec) + gather against SequenceScorer.score; ms per call, host clock between device "
                "syncs, legs alternated, median of reps; then the op alone between HIP events",
        "config": "java", "batch": a.batch, "nodes": a.nodes, "tokens": T, "vocab": V, "calls_per_rep": a.calls,
        "reps": a.reps, "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "groups": {}, "op": {},
    }
    g = torch.Generator().manual_seed(a.seed)
    cands = {}
    for G in GROUPS:
        cand = torch.randint(4, V, (a.batch, G, T), generator=g)
        ends = torch.randint(5, T, (a.batch, G), generator=g)
        col = torch.arange(T)[None, None, :]
        cand = torch.where(col == ends[:, :, None], torch.full_like(cand, EOS), cand)
        cands[G] = torch.where(col > ends[:, :, None], torch.full_like(cand, PAD), cand).to(dev)
    if a.fused:
        res["what"] = ("teacher-forced scoring of G candidates per AST from a precomputed encoder output, eval mode: "
                       "SequenceScorer(attention='fused') against attention='sdpa', forward under no_grad and forward + "
                       "backward; ms per call, host clock between device syncs, legs alternated, median of reps; then "
                       "seq_attention alone against SDPA with explicit masks between HIP events")
        fused_legs(a, model, enc, src_mask, cands, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.fused_out)), exist_ok=True)
        with open(a.fused_out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    for G in GROUPS:
        cand = cands[G]
        fns = {"generator": lambda: generator_leg(cand), "scorer": lambda: scorer.score(enc, src_mask, cand).logp}

        def run(leg, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                for _ in range(n):
                    fns[leg]()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        with torch.no_grad():
            diff = float((fns["generator"]() - fns["scorer"]()).abs().max())
        for leg in LEGS:  # warm-up: code objects, hipBLASLt heuristics, allocator
            run(leg, 2)
        ms = {leg: [] for leg in LEGS}
        for _ in range(a.reps):
            for leg in LEGS:
                ms[leg].append(run(leg, a.calls))
        out = {leg: summary(ms[leg]) for leg in LEGS}
        with torch.no_grad():
            for leg in LEGS:
                out[leg]["peak_bytes"] = peak_bytes(fns[leg])
        out["scorer_minus_generator_ms"] = out["scorer"]["median"] - out["generator"]["median"]
        out["resolved"] = resolved(out["scorer"], out["generator"])
        out["max_abs_difference_of_scores"] = diff
        out["rows"] = a.batch * G * T
        res["groups"][f"G={G}"] = out

        # the op alone at this (rows, V)
        rows = a.batch * G * T
        z = torch.randn(rows, V, device=dev)
        t = cand.reshape(-1)
        ops = {"token_logp": lambda zz: token_logp(zz, t, ignore_id=PAD),
               "log_softmax_gather": lambda zz: torch.log_softmax(zz, -1).gather(1, t[:, None])[:, 0]}
        zg = z.clone().requires_grad_()

        def fwd(fn):
            with torch.no_grad():
                return fn(z)

        def fwd_bwd(fn):
            zg.grad = None
            fn(zg).sum().backward()

        timed = {(name, k): (lambda fn=fn, f=f: f(fn)) for name, fn in ops.items()
                 for k, f in (("fwd_ms", fwd), ("fwd_bwd_ms", fwd_bwd))}
        op_ms = {key: [] for key in timed}
        for key, fn in timed.items():  # warm-up
            fn()
        for _ in range(a.reps):  # alternated, one event pair per call
            for key, fn in timed.items():
                op_ms[key] += events_ms(fn, 1)
        op_out = {name: {k: summary(op_ms[name, k]) for k in ("fwd_ms", "fwd_bwd_ms")} for name in ops}
        for name, fn in ops.items():
            zg.grad = None
            op_out[name]["fwd_peak_bytes"] = peak_bytes(lambda: fwd(fn))
            op_out[name]["fwd_bwd_peak_bytes"] = peak_bytes(lambda: fwd_bwd(fn))
        zg.grad = None
        del zg
        for k in ("fwd_ms", "fwd_bwd_ms"):
            op_out[k + "_resolved"] = resolved(op_out["token_logp"][k], op_out["log_softmax_gather"][k])
        op_out["rows"] = rows
        res["op"][f"G={G}"] = op_out
        del z

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
