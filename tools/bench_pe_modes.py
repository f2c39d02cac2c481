"""The train step at the config/java.py dims, 64 ASTs of 150 nodes, for each structure encoding (use_pegen): pegen
(the CSE layers, the headline configuration) and the four ablations. The laplacian mode runs three ways: the device
eigenvectors (csa_lap_pe, one workgroup per AST), the host fallback (lap_pe(..., backend="host"): per AST a
device-to-host copy and a LAPACK eigh, what the reference's encode() does on every call) and a precomputed data.lap_pe
(what a dataset layer would cache).

usage: python tools/bench_pe_modes.py [--batch 64] [--nodes 150] [--steps 3] [--reps 5] [--out profiles/pe_modes.json]

All legs live in one process on one GPU and are timed alternately: per rep, every leg runs `steps` train steps
(script/train.py:_update: forward, loss + sw * sparsity, GradScaler, fused AdamW) between two device synchronisations,
timed on the host clock, since the host leg's cost is host work. The JSON keeps the median of the reps, every rep and
the max - min spread per leg. The eigenvector kernel and the two tree-position kernels are also timed alone with HIP
events (median of `reps`). GEMMs come from the committed TunableOp table where it has the shape, as in bench.py's train
leg. Nothing is compared against a promise: the numbers are what they are. There is no CPU fallback: without a GPU the
tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import torch  # noqa: E402

LEGS = {  # leg -> (use_pegen, what differs from CONFIGS["java"], the batch's eigenvector source)
    "pegen": ("pegen", {}, None),
    "sequential": ("sequential", dict(pe_dim=0), None),
    "treepos": ("treepos", {}, None),
    "triplet": ("triplet", {}, None),
    "laplacian_device": ("laplacian", {}, "device"),
    "laplacian_host": ("laplacian", {}, "host"),
    "laplacian_precomputed": ("laplacian", {}, "precomputed"),
}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pe_modes.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pe_modes: needs the GPU (no CPU timing is meaningful)")
    import csa_amd.pe_ops as pe_ops
    from csa_amd import _lib
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CONFIGS, CSATrans, batch_to_device, label_smoothing_loss
    from csa_amd.train import AdamW, make_train_step, use_tuned_gemms

    dev = torch.device("cuda:0")
    ntuned = use_tuned_gemms(True)
    sb = synthetic_batch(a.batch, max_size=a.nodes, seed=a.seed, ablation_fields=True)
    pegen_dim = CONFIGS["java"]["pegen_dim"]
    steps, data = {}, {}
    for leg, (mode, over, source) in LEGS.items():
        torch.manual_seed(a.seed)
        model = CSATrans(**{**CONFIGS["java"], **over, "use_pegen": mode}).to(dev)
        opt = AdamW(model.parameters(), lr=1e-4, correct_bias=False)
        steps[leg] = make_train_step(model, opt, label_smoothing_loss, sw=1e-2, scaler=torch.amp.GradScaler("cuda"))
        x, y = batch_to_device(sb, dev)
        if source == "precomputed":
            x.lap_pe = pe_ops.lap_pe(x.adj, x.num_node, pegen_dim, check=True).pe
        data[leg] = (x, y, source)

    real_lap_pe = pe_ops.lap_pe

    def run(leg, n):
        x, y, source = data[leg]
        if source == "host":  # the model's encode() calls pe_ops.lap_pe: force the fallback for this leg alone
            pe_ops.lap_pe = lambda adj, nn_, dim, **kw: real_lap_pe(adj, nn_, dim, backend="host")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                steps[leg](x, y)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n
        finally:
            pe_ops.lap_pe = real_lap_pe

    for leg in LEGS:  # warm-up: code objects, hipBLASLt heuristics, allocator, the scaler's first steps
        run(leg, 2)
    ms = {leg: [] for leg in LEGS}
    for _ in range(a.reps):
        for leg in LEGS:
            ms[leg].append(run(leg, a.steps))

    # the kernels alone
    x = data["laplacian_device"][0]
    lap_ms, lap_all = events_ms(lambda: pe_ops.lap_pe(x.adj, x.num_node, pegen_dim), a.reps)
    r = pe_ops.lap_pe(x.adj, x.num_node, pegen_dim, check=True)
    t0 = time.perf_counter()
    pe_ops.lap_pe(x.adj, x.num_node, pegen_dim, backend="host")
    host_ms = (time.perf_counter() - t0) * 1e3
    F = pegen_dim // 128
    p = torch.empty(F, device=dev).uniform_(0.7, 0.999).requires_grad_(True)
    tp_fwd, tp_fwd_all = events_ms(lambda: pe_ops.tree_pos_encode(x.tree_pos, p, d_model=pegen_dim), a.reps)
    out = pe_ops.tree_pos_encode(x.tree_pos, p, d_model=pegen_dim)
    g = torch.randn_like(out)
    tp_bwd, tp_bwd_all = events_ms(lambda: torch.autograd.grad(out, p, g, retain_graph=True), a.reps)

    res = {
        "what": "train step (forward, loss + sw * sparsity, GradScaler, fused AdamW) per structure encoding; ms per step, "
                "host clock between device syncs, legs alternated, median of reps",
        "config": "java", "batch": a.batch, "nodes": a.nodes, "steps_per_rep": a.steps, "reps": a.reps,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "gemms": f"TunableOp table ({ntuned} shapes; other shapes on the hipBLASLt default)",
        "step_ms": {leg: statistics.median(v) for leg, v in ms.items()},
        "step_ms_all": ms,
        "step_ms_spread": {leg: max(v) - min(v) for leg, v in ms.items()},
        "kernels_ms": {
            "lap_pe_device": lap_ms, "lap_pe_device_all": lap_all, "lap_pe_host_once": host_ms,
            "lap_pe_sweeps_max": int(r.sweeps.max()), "lap_pe_status_nonzero": int((r.status != 0).sum()),
            "tree_pos_fwd": tp_fwd, "tree_pos_fwd_all": tp_fwd_all, "tree_pos_bwd": tp_bwd, "tree_pos_bwd_all": tp_bwd_all,
            "tree_pos_n_feat": F,
        },
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
