"""Greedy decoding at the config/java.py dims: GreedyGenerator (the reference loop, every step re-decodes all
tokens so far) against CachedGreedyGenerator (one position per step, KV cache, csrc/csa_decode.hip) and against
CachedGreedyGenerator(graph=True) (the same step, device-stepped and replayed as one captured HIP graph) on the same
weights and the same batch, in one process on one GPU.

usage: python tools/bench_greedy.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--reps 5] [--out profiles/greedy_decode.json]

Each generator is warmed up once (code objects, hipBLASLt heuristics, allocator; for the `graph` leg this is the call
that captures, timed on the host and reported as capture_ms), then the three are timed alternately `reps` times with
HIP events around the whole call (process_data + encode + all max_tgt_len-1 steps); the medians, the per-rep values
and the ratios go to the JSON. The `cached` leg is the yardstick of the `graph` leg: graph_beats_cached says whether the
graph median lies below the cached median by more than the cached leg's own max - min spread over the reps. The
encoder's graph sampling draws its Philox key from torch's CPU generator, so it is re-seeded before every call: all
generators then decode from the same encoder output, and the tool asserts that they return identical ids. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import torch  # noqa: E402


def graph_nodes(gen, data):
    """Nodes of the captured step, counted by the HIP runtime on a second, untimed capture that keeps its hipGraph_t
    (the timed generator's graph is instantiated the default way and keeps none). None when the runtime cannot say."""
    import ctypes

    from csa_amd.model import CachedGreedyGenerator
    try:
        probe = CachedGreedyGenerator(gen.model, gen.max_tgt_len, graph=True)
        probe._keep_graph = True
        probe(data)
        (entry,) = probe._graphs.values()
        with open("/proc/self/maps") as f:  # the HIP runtime torch has loaded, not a second copy of it
            path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
        hip = ctypes.CDLL(path)
        n = ctypes.c_size_t(0)
        hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        if hip.hipGraphGetNodes(ctypes.c_void_p(entry.graph.raw_cuda_graph()), None, ctypes.byref(n)) != 0:
            return None
        return int(n.value)
    except (AttributeError, OSError, RuntimeError, TypeError, StopIteration):
        return None


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
    gens = {"greedy": GreedyGenerator(model, a.max_tgt_len), "cached": CachedGreedyGenerator(model, a.max_tgt_len),
            "graph": CachedGreedyGenerator(model, a.max_tgt_len, graph=True)}

    def run(name):
        torch.manual_seed(a.seed)  # the same SBM sampling key for every call
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            start.record()
            ys = gens[name](data)
            stop.record()
        stop.synchronize()
        return ys, start.elapsed_time(stop)

    warm_ms = {}
    for name in gens:  # warm-up, outside the timed reps; the graph leg captures here
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(name)
        torch.cuda.synchronize()
        warm_ms[name] = (time.perf_counter() - t0) * 1e3
    assert gens["graph"].captures == 1
    ms = {name: [] for name in gens}
    ys = {}
    for _ in range(a.reps):
        for name in gens:
            ys[name], t = run(name)
            ms[name].append(t)
    identical = bool(torch.equal(ys["greedy"], ys["cached"]))
    identical_graph = identical and bool(torch.equal(ys["graph"], ys["cached"]))
    assert gens["graph"].captures == 1, "the timed graph calls recaptured"
    spread = max(ms["cached"]) - min(ms["cached"])
    med = {name: statistics.median(v) for name, v in ms.items()}
    res = {
        "what": "one greedy-decoded batch: process_data + encode + max_tgt_len-1 decode steps, HIP events, eval mode",
        "config": "java", "batch": a.batch, "nodes": a.nodes, "max_tgt_len": a.max_tgt_len, "reps": a.reps,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "greedy_ms": med["greedy"], "cached_ms": med["cached"], "speedup": med["greedy"] / med["cached"],
        "greedy_ms_all": ms["greedy"], "cached_ms_all": ms["cached"],
        "identical_ys": identical, "pad_tokens_generated": int((ys["greedy"] == 0).sum()),
        "graph_ms": med["graph"], "graph_ms_all": ms["graph"], "graph_speedup_over_cached": med["cached"] / med["graph"],
        "cached_spread_ms": spread, "graph_beats_cached": bool(med["cached"] - med["graph"] > spread),
        "capture_ms": warm_ms["graph"], "cached_warmup_ms": warm_ms["cached"], "graph_nodes": graph_nodes(gens["graph"], data),
        "replays_per_call": a.max_tgt_len - 1, "identical_ys_graph": identical_graph,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert identical, "CachedGreedyGenerator and GreedyGenerator returned different ids"
    assert identical_graph, "CachedGreedyGenerator(graph=True) returned different ids"


if __name__ == "__main__":
    main()
