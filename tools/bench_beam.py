"""Beam search at the config/java.py dims against the greedy step it is built on, in one process on one GPU:

  greedy_b    CachedGreedyGenerator(graph=True) on B ASTs;
  greedy_bw   the same on B * W ASTs: the decoder row count of the beam leg, its yardstick;
  beam        BeamSearchGenerator(graph=True), width W, on the B ASTs of greedy_b.

usage: python tools/bench_beam.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--beam 4] [--reps 5] [--out profiles/beam_decode.json]

Each leg is warmed up once (it captures its graph there), then the three are timed alternately `reps` times with HIP
events around the whole call (process_data + encode + all max_tgt_len-1 replays); medians and per-rep values go to the
JSON. greedy_bw encodes W times the ASTs of the beam leg, so process_data + encode alone is timed the same way at B and
at B * W and subtracted: the *_decode_ms figures are what the comparison is about. What lies between beam_decode_ms and
greedy_bw_decode_ms is the price of the selection plus the cache indirection (minus the memory projection the beam
shares); greedy_bw_spread_ms, the yardstick's own max - min over the reps, says how much of it is noise. The weights
are untrained, which changes no launch: every step runs at static shapes whatever the hypotheses hold. There is no CPU
fallback: without a GPU the tool fails."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CONFIGS, BeamSearchGenerator, CachedGreedyGenerator, CSATrans, batch_to_device

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    model = CSATrans(**CONFIGS["java"]).to(dev).eval()
    B, W, T = a.batch, a.beam, a.max_tgt_len

    def batch(n):
        data, _ = batch_to_device(synthetic_batch(n, max_size=a.nodes, seed=a.seed), dev)
        data.tgt_seq = None  # inference: no teacher-forced target side in process_data
        return data
    data = {"b": batch(B), "bw": batch(B * W)}
    greedy = CachedGreedyGenerator(model, T, graph=True)  # one generator, one graph per batch size
    beam = BeamSearchGenerator(model, T, W, graph=True)

    def encode(d):
        model.process_data(d)
        return model.encode(d)[0]
    legs = {"greedy_b": lambda: greedy(data["b"]), "greedy_bw": lambda: greedy(data["bw"]),
            "beam": lambda: beam(data["b"], return_all=True), "encode_b": lambda: encode(data["b"]),
            "encode_bw": lambda: encode(data["bw"])}

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
    assert greedy.captures == 2 and beam.captures == 1
    ms = {name: [] for name in legs}
    out = {}
    for _ in range(a.reps):
        for name in legs:
            out[name], t = run(name)
            ms[name].append(t)
    assert greedy.captures == 2 and beam.captures == 1, "a timed call recaptured"
    med = {name: statistics.median(v) for name, v in ms.items()}
    dec = {"greedy_b": med["greedy_b"] - med["encode_b"], "greedy_bw": med["greedy_bw"] - med["encode_bw"],
           "beam": med["beam"] - med["encode_b"]}
    best, ids, scores = out["beam"]
    res = {
        "what": "one decoded batch: process_data + encode + max_tgt_len-1 graph replays, HIP events, eval mode; "
                "*_decode_ms = the call minus process_data + encode timed alone at the same batch size",
        "config": "java", "batch": B, "beam": W, "rows": B * W, "nodes": a.nodes, "max_tgt_len": T, "reps": a.reps,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "greedy_b_ms": med["greedy_b"], "greedy_bw_ms": med["greedy_bw"], "beam_ms": med["beam"],
        "encode_b_ms": med["encode_b"], "encode_bw_ms": med["encode_bw"],
        "greedy_b_decode_ms": dec["greedy_b"], "greedy_bw_decode_ms": dec["greedy_bw"], "beam_decode_ms": dec["beam"],
        "beam_minus_greedy_bw_ms": med["beam"] - med["greedy_bw"],
        "beam_minus_greedy_bw_decode_ms": dec["beam"] - dec["greedy_bw"],
        "beam_over_greedy_b_decode": dec["beam"] / dec["greedy_b"],
        "greedy_bw_spread_ms": max(ms["greedy_bw"]) - min(ms["greedy_bw"]),
        "ms_all": ms,
        "beam_scores_ranked": bool((scores[:, :-1] >= scores[:, 1:]).all()),
        "beam_best_equals_greedy_b": bool(torch.equal(best, out["greedy_b"])),
        "replays_per_call": T - 1,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
