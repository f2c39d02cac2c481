"""Sampled decoding at the config/java.py dims against the greedy step it is built on, in one process on one GPU:

  greedy        CachedGreedyGenerator(graph=True) on B ASTs: the yardstick;
  sample        SamplingGenerator(graph=True), no filter (the single-pass kernel);
  sample_kp     SamplingGenerator(graph=True, top_k=40, top_p=0.9) (the radix-descent passes);
  sample_k      the same with top_k alone, and
  sample_p      with top_p alone: what each descent costs, end to end (in sample_kp the top-p passes see only the
                top-k set; in sample_p they see the whole row);
  sample_s      SamplingGenerator(graph=True, num_samples=S), no filter, B * S rows;
  beam          BeamSearchGenerator(W=S, graph=True): the other B * S-row strategy, the yardstick of sample_s.

usage: python tools/bench_sample.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--samples 4] [--reps 5]
                                    [--out profiles/sample_decode.json]

Each leg is warmed up once (it captures its graph there), then the legs are timed alternately `reps` times with HIP
events around the whole call (process_data + encode + all max_tgt_len-1 replays); medians and per-rep values go to the
JSON. Every leg encodes the same B ASTs, so the differences between legs are differences of the decode loop. Each
sampling leg is reported as its difference from the greedy leg of the same run beside its own spread (max - min over
the reps). The weights are untrained, which changes no launch: every step runs at static shapes whatever the rows hold.
Nothing is measured per kernel. There is no CPU fallback: without a GPU the tool fails."""
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
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import synthetic_batch
    from csa_amd.model import (CONFIGS, BeamSearchGenerator, CachedGreedyGenerator, CSATrans, SamplingGenerator,
                               batch_to_device)

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    model = CSATrans(**CONFIGS["java"]).to(dev).eval()
    B, S, T = a.batch, a.samples, a.max_tgt_len
    data, _ = batch_to_device(synthetic_batch(B, max_size=a.nodes, seed=a.seed), dev)
    data.tgt_seq = None  # inference: no teacher-forced target side in process_data
    gens = {"greedy": CachedGreedyGenerator(model, T, graph=True),
            "sample": SamplingGenerator(model, T, graph=True),
            "sample_kp": SamplingGenerator(model, T, top_k=a.top_k, top_p=a.top_p, graph=True),
            "sample_k": SamplingGenerator(model, T, top_k=a.top_k, graph=True),
            "sample_p": SamplingGenerator(model, T, top_p=a.top_p, graph=True),
            "sample_s": SamplingGenerator(model, T, num_samples=S, graph=True),
            "beam": BeamSearchGenerator(model, T, S, graph=True)}
    legs = {"greedy": lambda: gens["greedy"](data),
            "sample": lambda: gens["sample"](data, seed=a.seed, return_logp=True),
            "sample_kp": lambda: gens["sample_kp"](data, seed=a.seed, return_logp=True),
            "sample_k": lambda: gens["sample_k"](data, seed=a.seed, return_logp=True),
            "sample_p": lambda: gens["sample_p"](data, seed=a.seed, return_logp=True),
            "sample_s": lambda: gens["sample_s"](data, seed=a.seed, return_logp=True),
            "beam": lambda: gens["beam"](data, return_all=True)}

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
    ids, logp = out["sample"]
    ids_kp, logp_kp = out["sample_kp"]
    ids_s, logp_s = out["sample_s"]
    res = {
        "what": "one decoded batch: process_data + encode + max_tgt_len-1 graph replays, HIP events, eval mode; every leg "
                "encodes the same batch; *_minus_greedy_ms = the leg's median minus the greedy leg's of the same run, "
                "*_spread_ms = the leg's own max - min over the reps",
        "config": "java", "batch": B, "samples": S, "rows_s": B * S, "nodes": a.nodes, "max_tgt_len": T, "reps": a.reps,
        "top_k": a.top_k, "top_p": a.top_p, "vocab": CONFIGS["java"]["tgt_vocab_size"],
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "greedy_ms": med["greedy"], "sample_ms": med["sample"], "sample_kp_ms": med["sample_kp"],
        "sample_k_ms": med["sample_k"], "sample_p_ms": med["sample_p"],
        "sample_s_ms": med["sample_s"], "beam_ms": med["beam"],
        "greedy_spread_ms": spread["greedy"], "sample_spread_ms": spread["sample"],
        "sample_kp_spread_ms": spread["sample_kp"], "sample_k_spread_ms": spread["sample_k"],
        "sample_p_spread_ms": spread["sample_p"], "sample_s_spread_ms": spread["sample_s"],
        "beam_spread_ms": spread["beam"],
        "sample_minus_greedy_ms": med["sample"] - med["greedy"],
        "sample_kp_minus_greedy_ms": med["sample_kp"] - med["greedy"],
        "sample_kp_minus_sample_ms": med["sample_kp"] - med["sample"],
        "sample_k_minus_sample_ms": med["sample_k"] - med["sample"],
        "sample_p_minus_sample_ms": med["sample_p"] - med["sample"],
        "sample_s_minus_greedy_ms": med["sample_s"] - med["greedy"],
        "sample_s_minus_beam_ms": med["sample_s"] - med["beam"],
        "per_step_us": {name: 1000.0 * (med[name] - med["greedy"]) / (T - 1) for name in ("sample", "sample_kp", "sample_k", "sample_p")},
        "ms_all": ms,
        "sample_logp_finite": bool(torch.isfinite(logp).all()) and bool(torch.isfinite(logp_kp).all()),
        "logp_nonpositive": bool((logp <= 0).all()) and bool((logp_kp <= 0).all()) and bool((logp_s <= 0).all()),
        "sample_s_rows_differ": bool((ids_s[:, 0] != ids_s[:, 1]).any()) if S > 1 else None,
        "shapes": {"sample": list(ids.shape), "sample_kp": list(ids_kp.shape), "sample_s": list(ids_s.shape),
                   "sample_s_logp": list(logp_s.shape)},
        "replays_per_call": T - 1,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
