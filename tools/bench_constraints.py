"""Decoding constraints at the config/java.py dims against the same generators without them, in one process on one GPU:

  greedy   / greedy_c    CachedGreedyGenerator(graph=True) without and with constraints;
  beam     / beam_c      BeamSearchGenerator(W, graph=True) without and with constraints;
  sample   / sample_c    SamplingGenerator(graph=True) without and with constraints.

The constrained legs turn all four rules on (repetition penalty, no-repeat n-gram, minimum length, suppressed ids).

usage: python tools/bench_constraints.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--beam 4] [--reps 5]
                                         [--out profiles/constrain_decode.json]

Each leg is warmed up once (it captures its graph there), then the legs are timed alternately `reps` times with HIP
events around the whole call (process_data + encode + all max_tgt_len-1 replays); medians and per-rep values go to the
JSON. Every leg encodes the same B ASTs, so the difference between a constrained leg and its yardstick, the
unconstrained leg of the same generator in the same run, is the difference of the decode loop: one more graph node per
step, the constrain_rows launch. It is reported beside both legs' own spread (max - min over the reps); a difference
inside the spread says no more than that. The weights are untrained, which changes no launch: every step runs at static
shapes whatever the rows hold. Nothing is measured per kernel. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=150)
    ap.add_argument("--max-tgt-len", type=int, default=50)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_constraints: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import EOS, UNK, synthetic_batch
    from csa_amd.model import (CONFIGS, BeamSearchGenerator, CachedGreedyGenerator, CSATrans, DecodingConstraints,
                               SamplingGenerator, batch_to_device)

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    model = CSATrans(**CONFIGS["java"]).to(dev).eval()
    B, W, T = a.batch, a.beam, a.max_tgt_len
    data, _ = batch_to_device(synthetic_batch(B, max_size=a.nodes, seed=a.seed), dev)
    data.tgt_seq = None  # inference: no teacher-forced target side in process_data
    con = DecodingConstraints(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=5, suppress_ids=(UNK,), eos_id=EOS)
    gens = {"greedy": CachedGreedyGenerator(model, T, graph=True),
            "greedy_c": CachedGreedyGenerator(model, T, graph=True, constraints=con),
            "beam": BeamSearchGenerator(model, T, W, graph=True),
            "beam_c": BeamSearchGenerator(model, T, W, graph=True, constraints=con),
            "sample": SamplingGenerator(model, T, graph=True),
            "sample_c": SamplingGenerator(model, T, graph=True, constraints=con)}
    legs = {name: (lambda g=g: g(data, seed=a.seed)) if name.startswith("sample") else (lambda g=g: g(data))
            for name, g in gens.items()}

    def run(name):
        torch.manual_seed(a.seed)  # the same SBM sampling key for every call
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            start.record()
            out = legs[name]()
            stop.record()
        stop.synchronize()
        return out, start.elapsed_time(stop)

    for name in legs:  # warm-up, outside the timed reps; the graph legs capture here
        run(name)
    torch.cuda.synchronize()
    assert all(g.captures == 1 for g in gens.values())
    ms = {name: [] for name in legs}
    out = {}
    for _ in range(a.reps):
        for name in legs:
            out[name], t = run(name)
            ms[name].append(t)
    assert all(g.captures == 1 for g in gens.values()), "a timed call recaptured"
    med = {name: statistics.median(v) for name, v in ms.items()}
    spread = {name: max(v) - min(v) for name, v in ms.items()}

    def obeys(ids):  # what the constrained outputs may no longer hold, checked on the result of the last rep
        ids = ids.reshape(-1, T - 1).cpu()
        early = bool((ids[:, :con.min_length] == EOS).any())
        return {"no_suppressed_id": not bool((ids == UNK).any()), "no_eos_before_min_length": not early}

    base = ("greedy", "beam", "sample")
    res = {
        "what": "one decoded batch: process_data + encode + max_tgt_len-1 graph replays, HIP events, eval mode; every leg "
                "encodes the same batch; *_c = the same generator with all four constraint rules on; "
                "*_c_minus_*_ms = the constrained leg's median minus its unconstrained leg's of the same run, "
                "*_spread_ms = the leg's own max - min over the reps",
        "config": "java", "batch": B, "beam": W, "nodes": a.nodes, "max_tgt_len": T, "reps": a.reps,
        "vocab": CONFIGS["java"]["tgt_vocab_size"], "constraints": repr(con),
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        **{f"{name}_ms": med[name] for name in legs},
        **{f"{name}_spread_ms": spread[name] for name in legs},
        **{f"{b}_c_minus_{b}_ms": med[b + "_c"] - med[b] for b in base},
        "per_step_us": {b: 1000.0 * (med[b + "_c"] - med[b]) / (T - 1) for b in base},
        "inside_spread": {b: abs(med[b + "_c"] - med[b]) <= max(spread[b], spread[b + "_c"]) for b in base},
        "ms_all": ms,
        "constrained_outputs": {b: obeys(out[b + "_c"]) for b in base},
        "outputs_differ": {b: not torch.equal(out[b], out[b + "_c"]) for b in base},
        "replays_per_call": T - 1,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
