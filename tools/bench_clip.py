"""What global gradient-norm clipping costs in the train step at the config/java.py dims, 64 ASTs of 150 nodes, under
a GradScaler. Three legs:

  none   AdamW without clipping (the step as bench.py times it)
  fused  AdamW(max_grad_norm=1.0): csa_grad_sumsq + csa_grad_norm_finish in front of the clipped csa_adamw_step
  torch  scaler.unscale_(opt); torch.nn.utils.clip_grad_norm_(params, 1.0) in front of the unclipped AdamW

usage: python tools/bench_clip.py [--batch 64] [--nodes 150] [--steps 3] [--reps 5] [--out profiles/grad_clip.json]

All legs live in one process on one GPU and are timed alternately: per rep, every leg runs `steps` train steps
(script/train.py:_update: forward, loss + sw * sparsity, GradScaler, AdamW) between two device synchronisations on the
host clock. The JSON keeps the median of the reps, every rep and the max - min spread per leg, and says whether the
fused leg is resolved from the none leg by more than their spreads. The optimizer part alone (on the gradients the last
step left, no scaler, so the torch leg has no unscale_ pass there) is timed with HIP events as well. GEMMs come from
the committed TunableOp table where it has the shape, as in bench.py's train leg. Nothing is compared against a
promise: the numbers are what they are. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import torch  # noqa: E402

LEGS = ("none", "fused", "torch")
MAX_NORM = 1.0


def make_torch_clip_step(model, optimizer, loss_fn, sw, scaler):
    """make_train_step's step with the stock clipping recipe in front of the optimizer."""
    params = [p for p in model.parameters() if p.requires_grad]

    def step(x, y):
        model.train(True)
        optimizer.zero_grad(set_to_none=True)
        y_pred, sparsity, *_ = model(x)
        loss = loss_fn(y_pred, y)
        scaler.scale(loss + sw * sparsity).backward()
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        scaler.step(optimizer)
        scaler.update()
        return loss.detach()

    return step


def events_ms(fn, reps):
    """Median, and all, of `reps` HIP-event timings of fn() after one warm-up call."""
    fn()
    out = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=150)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CONFIGS, CSATrans, batch_to_device, label_smoothing_loss
    from csa_amd.train import AdamW, make_train_step, use_tuned_gemms

    dev = torch.device("cuda:0")
    ntuned = use_tuned_gemms(True)
    x, y = batch_to_device(synthetic_batch(a.batch, max_size=a.nodes, seed=a.seed), dev)
    steps, opts, models = {}, {}, {}
    for leg in LEGS:
        torch.manual_seed(a.seed)
        model = CSATrans(**CONFIGS["java"]).to(dev)
        opt = AdamW(model.parameters(), lr=1e-4, correct_bias=False, max_grad_norm=MAX_NORM if leg == "fused" else None)
        scaler = torch.amp.GradScaler("cuda")
        if leg == "torch":
            steps[leg] = make_torch_clip_step(model, opt, label_smoothing_loss, 1e-2, scaler)
        else:
            steps[leg] = make_train_step(model, opt, label_smoothing_loss, sw=1e-2, scaler=scaler)
        opts[leg], models[leg] = opt, model

    def run(leg, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            steps[leg](x, y)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for leg in LEGS:  # warm-up: code objects, hipBLASLt heuristics, allocator, the scaler's first steps
        run(leg, 2)
    ms = {leg: [] for leg in LEGS}
    for _ in range(a.reps):
        for leg in LEGS:
            ms[leg].append(run(leg, a.steps))
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    spread = {leg: max(v) - min(v) for leg, v in ms.items()}

    norm, coef = float(opts["fused"].last_grad_norm), float(opts["fused"].last_clip_coef)  # of the last timed step

    # the optimizer part alone, on the gradients of the last step
    params = [p for p in models["torch"].parameters() if p.grad is not None]

    def torch_clip_then_step():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opts["torch"].step()

    opt_ms = {}
    for leg, fn in (("none", opts["none"].step), ("fused", opts["fused"].step), ("torch", torch_clip_then_step)):
        opt_ms[leg], opt_ms[leg + "_all"] = events_ms(fn, a.reps)

    nparam = sum(p.numel() for p in models["none"].parameters())
    res = {
        "what": "train step (forward, loss + sw * sparsity, GradScaler, AdamW) without clipping, with the fused "
                "max_grad_norm=1.0, and with scaler.unscale_ + torch clip_grad_norm_ in front of the unclipped AdamW; "
                "ms per step, host clock between device syncs, legs alternated, median of reps",
        "config": "java", "batch": a.batch, "nodes": a.nodes, "steps_per_rep": a.steps, "reps": a.reps,
        "max_grad_norm": MAX_NORM, "parameters": nparam,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "gemms": f"TunableOp table ({ntuned} shapes; other shapes on the hipBLASLt default)",
        "step_ms": med, "step_ms_all": ms, "step_ms_spread": spread,
        "fused_minus_none_ms": med["fused"] - med["none"],
        "torch_minus_none_ms": med["torch"] - med["none"],
        "fused_resolved_from_none": abs(med["fused"] - med["none"]) > max(spread["fused"], spread["none"]),
        "torch_resolved_from_fused": abs(med["torch"] - med["fused"]) > max(spread["torch"], spread["fused"]),
        "optimizer_only_ms": opt_ms,
        "optimizer_only_what": "HIP events around the optimizer part alone on the last step's gradients, no scaler: "
                               "AdamW.step(), AdamW(max_grad_norm).step(), clip_grad_norm_ + AdamW.step() (no unscale_ "
                               "pass); median of reps after one warm-up call",
        "last_grad_norm": norm, "last_clip_coef": coef,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
