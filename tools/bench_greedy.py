"""Greedy decoding at the config/java.py dims: GreedyGenerator (the reference loop, every step re-decodes all
tokens so far) against CachedGreedyGenerator (one position per step, KV cache, csrc/csa_decode.hip) on the same
weights and the same batch, in one process on one GPU.

usage: python tools/bench_greedy.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--reps 5] [--out profiles/greedy_decode.json]

Each generator is warmed up once (code objects, hipBLASLt heuristics, allocator), then the two are timed alternately
`reps` times with HIP events around the whole call (process_data + encode + all max_tgt_len-1 steps); the medians and
their ratio go to the JSON. The encoder's graph sampling draws its Philox key from torch's CPU generator, so it is
re-seeded before every call: both generators then decode from the same encoder output, and the tool asserts that they
return identical ids. There is no CPU fallback: without a GPU the tool fails."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_greedy: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CONFIGS, CachedGreedyGenerator, CSATrans, GreedyGenerator, batch_to_device

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    model = CSATrans(**CONFIGS["java"]).to(dev).eval()
    data, _ = batch_to_device(synthetic_batch(a.batch, max_size=a.nodes, seed=a.seed), dev)
    data.tgt_seq = None  # inference: no teacher-forced target side in process_data
    gens = {"greedy": GreedyGenerator(model, a.max_tgt_len), "cached": CachedGreedyGenerator(model, a.max_tgt_len)}

    def run(name):
        torch.manual_seed(a.seed)  # the same SBM sampling key for every call
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            start.record()
            ys = gens[name](data)
            stop.record()
        stop.synchronize()
        return ys, start.elapsed_time(stop)

    for name in gens:  # warm-up, untimed
        run(name)
    ms = {name: [] for name in gens}
    ys = {}
    for _ in range(a.reps):
        for name in gens:
            ys[name], t = run(name)
            ms[name].append(t)
    identical = bool(torch.equal(ys["greedy"], ys["cached"]))
    med = {name: statistics.median(v) for name, v in ms.items()}
    res = {
        "what": "one greedy-decoded batch: process_data + encode + max_tgt_len-1 decode steps, HIP events, eval mode",
        "config": "java", "batch": a.batch, "nodes": a.nodes, "max_tgt_len": a.max_tgt_len, "reps": a.reps,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "greedy_ms": med["greedy"], "cached_ms": med["cached"], "speedup": med["greedy"] / med["cached"],
        "greedy_ms_all": ms["greedy"], "cached_ms_all": ms["cached"],
        "identical_ys": identical, "pad_tokens_generated": int((ys["greedy"] == 0).sum()),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert identical, "CachedGreedyGenerator and GreedyGenerator returned different ids"


if __name__ == "__main__":
    main()
