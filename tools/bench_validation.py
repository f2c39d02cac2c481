"""One validation batch at the config/java.py dims: what scoring the decoded ids costs on top of decoding them, on the
device (csa_amd.metrics.SummaryMetrics, csrc/csa_metric.hip) and on the host (ids copied to the host, then the
per-sentence Counter / DP loops of tests/metric_ref.py, which restate the reference's BLEU4 and ROUGE-L code).

usage: python tools/bench_validation.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--reps 5]
                                        [--out profiles/validation_metrics.json]

Three legs on the same weights, batch and targets, CachedGreedyGenerator(graph=True), timed alternately `reps` times
after one warm-up each (the graph leg captures there), wall clock between two device synchronisations:
  decode         ys = generator(data)
  decode_device  the same, then SummaryMetrics.update(ys, target): one launch and two small reductions, no host copy
  decode_host    the same, then ys.cpu() and metric_ref.score over the rows (the host leg skips the reference's
                 id -> word mapping and its per-id .item() calls, which only makes it cheaper than the reference's)
Medians, per-rep values and max - min spreads go to the JSON, with each scoring leg's excess over decode alone; the
seq_metrics call alone is timed between HIP events over `--metric-reps` back-to-back calls (metric_launch_ms: the
call's launch-path latency, not the kernel's duration). The tool asserts that both
scoring legs report the same numbers. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=150)
    ap.add_argument("--max-tgt-len", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metric-reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_metrics.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation: needs the GPU (no CPU timing is meaningful)")
    import metric_ref
    from csa_amd import _lib
    from csa_amd.data import EOS, synthetic_batch
    from csa_amd.metric_ops import seq_metrics
    from csa_amd.metrics import SummaryMetrics
    from csa_amd.model import CONFIGS, CachedGreedyGenerator, CSATrans, batch_to_device

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    model = CSATrans(**CONFIGS["java"]).to(dev).eval()
    data, target = batch_to_device(synthetic_batch(a.batch, max_size=a.nodes, seed=a.seed, max_tgt_len=a.max_tgt_len), dev)
    data.tgt_seq = None  # inference: no teacher-forced target side in process_data
    gen = CachedGreedyGenerator(model, a.max_tgt_len, graph=True)
    target_host = target.cpu().numpy()
    results = {}

    def decode():
        torch.manual_seed(a.seed)  # the same SBM sampling key for every call
        with torch.no_grad():
            return gen(data)

    def leg_decode():
        decode()

    def leg_device():
        sm = SummaryMetrics(EOS)
        sm.update(decode(), target)
        results["device"] = sm  # read after the clock stops

    def leg_host():
        ys = decode().cpu().numpy()
        results["host"] = metric_ref.aggregate(*metric_ref.score(ys, target_host, EOS, 1))

    legs = {"decode": leg_decode, "decode_device": leg_device, "decode_host": leg_host}

    def run(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        legs[name]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    warm_ms = {name: run(name) for name in legs}
    assert gen.captures == 1
    ms = {name: [] for name in legs}
    for _ in range(a.reps):
        for name in legs:
            ms[name].append(run(name))
    assert gen.captures == 1, "the timed calls recaptured"
    d, h = results["device"].compute(), results["host"]
    same = d.n == h["n"] and all(abs(getattr(d, k) - h[k]) <= 1e-12 for k in ("bleu", "corpus_bleu", "rouge_l"))

    ys = decode()
    ev = []
    for _ in range(a.metric_reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        seq_metrics(ys, target, eos_id=EOS, backend="device")
        stop.record()
        stop.synchronize()
        ev.append(start.elapsed_time(stop))

    med = {name: statistics.median(v) for name, v in ms.items()}
    spread = {name: max(v) - min(v) for name, v in ms.items()}
    dev_excess, host_excess = med["decode_device"] - med["decode"], med["decode_host"] - med["decode"]
    res = {
        "what": "one validation batch: greedy decode (captured graph) alone, plus the device metric, plus the host loops; "
                "wall clock between device synchronisations, eval mode",
        "config": "java", "batch": a.batch, "nodes": a.nodes, "max_tgt_len": a.max_tgt_len, "reps": a.reps,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "decode_ms": med["decode"], "decode_device_ms": med["decode_device"], "decode_host_ms": med["decode_host"],
        "decode_ms_all": ms["decode"], "decode_device_ms_all": ms["decode_device"], "decode_host_ms_all": ms["decode_host"],
        "spread_ms": spread, "warmup_ms": warm_ms,
        "device_excess_ms": dev_excess, "host_excess_ms": host_excess,
        "device_excess_is_smaller": bool(dev_excess < host_excess),
        "excess_above_decode_spread": {"device": bool(dev_excess > spread["decode"]), "host": bool(host_excess > spread["decode"])},
        "metric_launch_ms": statistics.median(ev), "metric_launch_ms_all": ev, "metric_rows": int(ys.shape[0]),
        "metric_widths": [int(ys.shape[1]), int(target.shape[1])],
        "scores": {"bleu": d.bleu, "corpus_bleu": d.corpus_bleu, "rouge_l": d.rouge_l, "n": d.n},
        "device_and_host_scores_agree": bool(same),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert same, "the device metric and the host loops disagree"


if __name__ == "__main__":
    main()
