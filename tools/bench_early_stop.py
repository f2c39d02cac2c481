"""Early stop at EOS at the config/java.py dims against the same generators without it, in one process on one GPU:
CachedGreedyGenerator(eos_id=EOS), BeamSearchGenerator(W) and SamplingGenerator, all graph=True.

usage: python tools/bench_early_stop.py [--batch 64] [--nodes 150] [--max-tgt-len 50] [--beam 4] [--reps 5]
                                        [--out profiles/early_stop_decode.json]

How much a corpus saves depends only on the step at which the last row of a batch finishes, so that step is what the
legs set: leg L raises generator.linear.bias[EOS] by --eos-bias and bans EOS below step L with
DecodingConstraints(min_length=L), so every row emits EOS at step L and the rule runs L + 2 steps; the leg `never` keeps
the bias as it is and bans EOS at every step, so nothing finishes and all max_tgt_len - 1 steps run. Each leg has two
generators that differ in early_stop alone (same constraints, so the same launches per step but for the counter's
increment, which early_stop replaces by csa_decode_advance). After one warm-up call each (the graphs are captured
there) the two are timed alternately `reps` times with HIP events around the whole call (process_data + encode + the
replays + the final read of the latch); wall-clock times of the same calls are kept beside them. Medians, spreads
(max - min over the reps), last_steps_run and last_replays go to the JSON, with the saving of each leg (off - on)
beside both spreads, the overhead of the never-finishing leg, and a least-squares line of the early-stopping medians
over the steps run (the cost per step run). A difference inside the spreads says no more than that. The same A/B at
L = 15 with poll_every in {2, 4, 8} is recorded as `poll_every`; the calls of that A/B run the same steps and differ in
parked replays alone, which gives `us_per_parked_replay` (a parked replay stores nothing but still runs the step's
GEMMs). The weights are untrained, which changes no launch. Nothing is measured per kernel. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import torch  # noqa: E402

LEGS = (5, 15, 30)
POLLS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=150)
    ap.add_argument("--max-tgt-len", type=int, default=50)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--eos-bias", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_early_stop: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import EOS, synthetic_batch
    from csa_amd.model import (CONFIGS, BeamSearchGenerator, CachedGreedyGenerator, CSATrans, DecodingConstraints,
                               SamplingGenerator, batch_to_device)

    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    model = CSATrans(**CONFIGS["java"]).to(dev).eval()
    B, W, T = a.batch, a.beam, a.max_tgt_len
    data, _ = batch_to_device(synthetic_batch(B, max_size=a.nodes, seed=a.seed), dev)
    data.tgt_seq = None  # inference: no teacher-forced target side in process_data
    bias = model.generator.linear.bias
    bias0 = float(bias[EOS].detach())

    def make(kind, con, early_stop):
        if kind == "greedy":
            g = CachedGreedyGenerator(model, T, graph=True, constraints=con, eos_id=EOS, early_stop=early_stop)
            return g, lambda: g(data)
        if kind == "beam":
            g = BeamSearchGenerator(model, T, W, graph=True, constraints=con, early_stop=early_stop)
            return g, lambda: g(data)
        g = SamplingGenerator(model, T, graph=True, constraints=con, early_stop=early_stop)
        return g, lambda: g(data, seed=a.seed)

    kinds = ("greedy", "beam", "sample")
    legs = {}  # (kind, leg name) -> {"off": (gen, call), "on": (gen, call), "bias": value of bias[EOS]}
    for kind in kinds:
        for L in LEGS + ("never",):
            con = DecodingConstraints(min_length=T if L == "never" else L, eos_id=EOS)
            legs[kind, str(L)] = {"off": make(kind, con, False), "on": make(kind, con, True),
                                  "bias": bias0 if L == "never" else bias0 + a.eos_bias}

    def run(leg, which):
        gen, call = leg[which]
        with torch.no_grad():
            bias[EOS] = leg["bias"]  # in place: the captured graphs read the weights where they are
        torch.manual_seed(a.seed)  # the same SBM sampling key for every call
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        with torch.no_grad():
            start.record()
            out = call()
            stop.record()
        stop.synchronize()
        wall = 1000.0 * (time.perf_counter() - t0)
        return out, start.elapsed_time(stop), wall, gen.last_steps_run, gen.last_replays

    def ab(leg, reps, polls=(None,)):
        """Alternating reps of the leg's two generators (the early-stopping one once per poll_every) -> records."""
        rec = {"off": {"ms": [], "wall_ms": []}}
        for p in polls:
            rec["on" if p is None else f"on_poll{p}"] = {"ms": [], "wall_ms": []}
        same = True
        for _ in range(reps):
            want, ms, wall, steps, replays = run(leg, "off")
            rec["off"]["ms"].append(ms)
            rec["off"]["wall_ms"].append(wall)
            rec["off"].update(steps_run=steps, replays=replays)
            for p in polls:
                if p is not None:
                    leg["on"][0].poll_every = p
                got, ms, wall, steps, replays = run(leg, "on")
                r = rec["on" if p is None else f"on_poll{p}"]
                r["ms"].append(ms)
                r["wall_ms"].append(wall)
                r.update(steps_run=steps, replays=replays, poll_every=leg["on"][0].poll_every)
                same = same and torch.equal(got, want)
        for r in rec.values():
            r["median_ms"], r["spread_ms"] = statistics.median(r["ms"]), max(r["ms"]) - min(r["ms"])
            r["median_wall_ms"] = statistics.median(r["wall_ms"])
        rec["bitwise_equal"] = same
        return rec

    for leg in legs.values():  # warm-up, outside the timed reps; the graphs are captured here
        run(leg, "off")
        run(leg, "on")
    torch.cuda.synchronize()
    res_legs, res_poll, fit = {}, {}, {}
    for kind in kinds:
        res_legs[kind] = {}
        for L in LEGS + ("never",):
            rec = ab(legs[kind, str(L)], a.reps)
            off, on = rec["off"], rec["on"]
            rec["saving_ms"] = off["median_ms"] - on["median_ms"]
            rec["saving_wall_ms"] = off["median_wall_ms"] - on["median_wall_ms"]
            rec["inside_spread"] = abs(rec["saving_ms"]) <= max(off["spread_ms"], on["spread_ms"])
            res_legs[kind][str(L)] = rec
        # the line through (steps run, median of the early-stopping leg): its slope is the cost of one step run
        xs = [res_legs[kind][str(L)]["on"]["steps_run"] for L in LEGS + ("never",)]
        ys = [res_legs[kind][str(L)]["on"]["median_ms"] for L in LEGS + ("never",)]
        mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
        slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
        fit[kind] = {"us_per_step_run": 1000.0 * slope, "intercept_ms": my - slope * mx, "steps_run": xs, "median_ms": ys}
        default = legs[kind, "15"]["on"][0].POLL_EVERY
        res_poll[kind] = ab(legs[kind, "15"], a.reps, POLLS)
        legs[kind, "15"]["on"][0].poll_every = default
    with torch.no_grad():
        bias[EOS] = bias0
    gens = [leg[w][0] for leg in legs.values() for w in ("off", "on")]
    assert all(g.captures == 1 for g in gens), "a timed call recaptured"
    poll_total = {p: sum(res_poll[k][f"on_poll{p}"]["median_ms"] for k in kinds) for p in POLLS}
    parked = {}  # the same steps run under two chunk sizes differ in parked replays alone
    for k in kinds:
        lo, hi = res_poll[k][f"on_poll{POLLS[0]}"], res_poll[k][f"on_poll{POLLS[-1]}"]
        if hi["replays"] > lo["replays"]:
            parked[k] = 1000.0 * (hi["median_ms"] - lo["median_ms"]) / (hi["replays"] - lo["replays"])
    res = {
        "what": "one decoded batch: process_data + encode + the graph replays, HIP events (and wall-clock), eval mode; "
                "every leg encodes the same batch; leg L: every row emits EOS at step L (EOS bias raised, min_length=L), "
                "leg never: EOS banned at every step; off / on = early_stop False / True of the same generator and "
                "constraints, timed alternately; saving_ms = median off - median on; spread_ms = max - min over the reps; "
                "fit = least-squares line of the on medians over the steps run; poll_every = the L = 15 leg with "
                "poll_every 2, 4 and 8, alternately; us_per_parked_replay = (median at 8 - median at 2) / (replays at 8 - "
                "replays at 2); the fitted line's steps include each leg's few parked replays (replays - steps_run)",
        "config": "java", "batch": B, "beam": W, "nodes": a.nodes, "max_tgt_len": T, "reps": a.reps,
        "vocab": CONFIGS["java"]["tgt_vocab_size"], "eos_bias": a.eos_bias,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "default_poll_every": gens[0].POLL_EVERY,
        "legs": res_legs, "fit": fit, "poll_every": res_poll,
        "poll_every_sum_of_medians_ms": {str(p): v for p, v in poll_total.items()},
        "us_per_parked_replay": parked,
        "per_kernel_time": "not measured",
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {k: {L: {"off": round(r["off"]["median_ms"], 3), "on": round(r["on"]["median_ms"], 3),
                     "steps": r["on"]["steps_run"], "replays": r["on"]["replays"], "equal": r["bitwise_equal"]}
                 for L, r in v.items()} for k, v in res_legs.items()}
    print(json.dumps({"legs": brief, "fit": {k: round(v["us_per_step_run"], 1) for k, v in fit.items()},
                      "poll_every_sum_of_medians_ms": res["poll_every_sum_of_medians_ms"]}))


if __name__ == "__main__":
    main()
