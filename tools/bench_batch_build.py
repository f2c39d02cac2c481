"""What batch preparation costs, on the host and on the device, for batches of 150-node ASTs (B = 64 and 256).

Legs per batch size, all in one process on one GPU, timed alternately (per rep every leg once), median of the reps
with every rep and the max - min spread kept:

  prep, pegen fields (L, T, L_mask, T_mask), ms per batch on the host clock, ending in a device synchronisation:
    host     data.relation_planes on 16 threads + the copy of the four planes to the device
    device   the copy of parents and num_node + batch_ops.ast_batch
  prep, treepos field (tree_pos): data.tree_positions per AST + the copy, against parents + ast_batch(("tree_pos",))
  kernel   csa_ast_batch alone (the C entry point on resident parents and preallocated outputs, 10 launches between
           two HIP events, ms per launch): the four planes, tree_pos, all seven fields
  step     the config/java.py train step (forward, loss + sw * sparsity, GradScaler, AdamW), use_pegen "pegen" and
           "treepos", fed per step by a batch built on the host and copied (model.batch_to_device of the full dict), by
           a parents-only batch (batch_to_device of synthetic_batch(planes=False)'s dict; CSATrans.process_data builds
           the fields on the device), and by a batch that is already resident (what bench.py times)

and once, at N = 1024 (B = 8): the kernel alone for the four planes and for triplet alone, the latter being the table
setup (three O(n) passes by single lanes) with next to nothing to write.

usage: python tools/bench_batch_build.py [--batches 64,256] [--nodes 150] [--steps 2] [--reps 5] [--out profiles/batch_build.json]

Nothing is compared against a promise: the numbers are what they are. There is no CPU fallback: without a GPU the tool
fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "code-structure-aware-transformer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PLANES = ("L", "T", "L_mask", "T_mask")
ALL = PLANES + ("adj", "tree_pos", "triplet")


def summary(ms):
    return {"median": statistics.median(ms), "all": ms, "spread": max(ms) - min(ms)}


def alternate(legs, reps, warm=1):
    """legs: {name: fn() -> ms}. Every leg once per rep, in turn, after `warm` untimed rounds."""
    for _ in range(warm):
        for fn in legs.values():
            fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(fn())
    return {k: summary(v) for k, v in ms.items()}


def host_ms(fn):
    """fn() between two device synchronisations on the host clock."""
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    return run


def event_ms(fn, per=1):
    """fn() between two HIP events, divided by the `per` launches it enqueues."""
    def run():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / per
    return run


KERNEL_LAUNCHES = 10  # launches between a pair of events of the kernel-alone legs


def raw_kernel(par, nn, fields):
    """csa_ast_batch itself on resident inputs and preallocated outputs (no Python, allocation or other kernel
    between the events): fn() enqueues KERNEL_LAUNCHES launches; the leg reports ms per launch."""
    import ctypes

    from csa_amd import _lib
    from csa_amd.batch_ops import ast_batch
    o = ast_batch(par, nn, fields=fields, backend="device")  # the buffers, laid out as ast_batch lays them out
    B, N = par.shape
    args = _lib.AstBatchArgs(B=B, N=N, parents=par.data_ptr(), num_node=nn.data_ptr(), status=o.status.data_ptr(),
                             plane_sb=2 * N * N if hasattr(o, "rel") or hasattr(o, "rel_mask") else 0)
    for f in fields:
        setattr(args, f, getattr(o, f).data_ptr())
    L, st = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        for _ in range(KERNEL_LAUNCHES):
            _lib.check(L.csa_ast_batch(ctypes.byref(args), st), "csa_ast_batch")
    fn.keep = (o, par, nn)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--nodes", type=int, default=150)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the train-step legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_build.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_build: needs the GPU (no CPU timing is meaningful)")
    from csa_amd import _lib
    from csa_amd.batch_ops import ast_batch
    from csa_amd.data import relation_planes, synthetic_batch, tree_positions
    from csa_amd.model import CONFIGS, CSATrans, batch_to_device, label_smoothing_loss
    from csa_amd.train import AdamW, make_train_step, use_tuned_gemms

    dev = torch.device("cuda:0")
    N = a.nodes
    ntuned = use_tuned_gemms(True)
    threads = min(16, os.cpu_count() or 1)
    res = {
        "what": "batch preparation on the host (relation_planes / tree_positions + copies) against the device "
                "(copy of parents + csa_ast_batch), the kernel alone, and the java train step fed either way; ms, legs "
                "alternated in one process, median of reps with every rep and the max - min spread",
        "nodes": N, "reps": a.reps, "steps_per_rep": a.steps, "host_threads": threads,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.loaded_source_hash(),
        "gemms": f"TunableOp table ({ntuned} shapes; other shapes on the hipBLASLt default)", "batch": {},
    }

    models = {}
    if not a.no_step:
        for mode in ("pegen", "treepos"):
            torch.manual_seed(a.seed)
            model = CSATrans(**{**CONFIGS["java"], "use_pegen": mode}).to(dev)
            opt = AdamW(model.parameters(), lr=1e-4, correct_bias=False)
            models[mode] = make_train_step(model, opt, label_smoothing_loss, sw=1e-2, scaler=torch.amp.GradScaler("cuda"))

    for B in (int(b) for b in a.batches.split(",")):
        full = synthetic_batch(B, max_size=N, seed=a.seed, min_nodes=N // 3, max_nodes=N, ablation_fields=True)
        slim = synthetic_batch(B, max_size=N, seed=a.seed, min_nodes=N // 3, max_nodes=N, planes=False)
        par, nn = slim["parents"], slim["num_node"].astype(np.int32)
        up = lambda x: torch.from_numpy(x).to(dev, non_blocking=True)
        r = {"bytes": {"parents_and_num_node": int(par.nbytes + nn.nbytes), "four_planes": 4 * B * N * N,
                       "tree_pos": B * N * 128 * 4}}

        def host_planes():
            return [up(x) for x in relation_planes(par, nn, N, nthreads=threads)]

        def device_planes():
            return ast_batch(up(par), up(nn))

        def host_treepos():
            return up(np.stack([tree_positions(par[b, :nn[b]].astype(np.int64), N) for b in range(B)]))

        def device_treepos():
            return ast_batch(up(par), up(nn), fields=("tree_pos",))

        r["prep_ms"] = alternate({"host_planes": host_ms(host_planes), "device_planes": host_ms(device_planes),
                                  "host_treepos": host_ms(host_treepos), "device_treepos": host_ms(device_treepos)},
                                 a.reps)
        dpar, dnn = up(par), up(nn)
        r["kernel_ms"] = alternate({k: event_ms(raw_kernel(dpar, dnn, f), KERNEL_LAUNCHES) for k, f in
                                    (("planes", PLANES), ("tree_pos", ("tree_pos",)), ("all_fields", ALL))}, a.reps)

        for mode, step in models.items():
            keys = PLANES if mode == "pegen" else ("tree_pos",)
            base = {k: v for k, v in full.items() if k in ("src_seq", "tgt_seq", "target", "src_mask")}

            def host_fed():  # what a loader thread and the copy do today, then the step
                if mode == "pegen":
                    built = dict(zip(PLANES, relation_planes(par, nn, N, nthreads=threads)))
                else:  # the hot-path planes are not read in this mode, but batch_to_device ships them: the resident ones
                    built = {k: full[k] for k in PLANES}
                    built["tree_pos"] = np.stack([tree_positions(par[b, :nn[b]].astype(np.int64), N) for b in range(B)])
                x, y = batch_to_device({**base, **built}, dev)
                return step(x, y)

            def device_fed():
                x, y = batch_to_device(slim, dev)
                return step(x, y)

            resident = batch_to_device({**base, **{k: full[k] for k in PLANES + keys}}, dev)

            def resident_fed():
                x, y = resident
                return step(type(x)(**{k: getattr(x, k) for k in ("src_seq", "tgt_seq") + PLANES + keys}), y)

            def many(fn):
                def run():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3 / a.steps
                return run

            r[f"step_ms_{mode}"] = alternate({"host_fed": many(host_fed), "device_fed": many(device_fed),
                                              "resident": many(resident_fed)}, a.reps, warm=2)
        res["batch"][str(B)] = r

    # the long-AST size: what the single-lane table setup costs
    NL, BL = 1024, 8
    long_ = synthetic_batch(BL, max_size=NL, seed=a.seed, planes=False)
    lp, ln = torch.from_numpy(long_["parents"]).to(dev), torch.from_numpy(long_["num_node"].astype(np.int32)).to(dev)
    res["long"] = {"nodes": NL, "batch": BL,
                   "kernel_ms": alternate({"planes": event_ms(raw_kernel(lp, ln, PLANES), KERNEL_LAUNCHES),
                                           "triplet_only": event_ms(raw_kernel(lp, ln, ("triplet",)), KERNEL_LAUNCHES)},
                                          a.reps)}
    short = synthetic_batch(BL, max_size=N, seed=a.seed, planes=False)
    sp, sn = torch.from_numpy(short["parents"]).to(dev), torch.from_numpy(short["num_node"].astype(np.int32)).to(dev)
    res["setup_at_nodes"] = {"nodes": N, "batch": BL, "kernel_ms": alternate(
        {"triplet_only": event_ms(raw_kernel(sp, sn, ("triplet",)), KERNEL_LAUNCHES)}, a.reps)}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
