"""Batch preparation on the device (csrc/csa_batch.hip): every structural field of a batch of ASTs from their parent
arrays.

ast_batch turns parents (B, N) and num_node (B) into the relation planes the hot path reads (L, T, L_mask, T_mask) and
the fields of the use_pegen ablations (adj, tree_pos, triplet) in one launch, instead of building them on the host
(data.relation_planes, data.adjacency / tree_positions / triplet_ids) and copying 90-170 KB per AST to the device. CPU
tensors, sizes the kernel does not support and backend="host" take exactly those host builders.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import data as _data
from ._lib import AstBatchArgs, CsaError, lib, on_device
from ._lib import check as _check

_vp = ctypes.c_void_p

PLANES = ("L", "T", "L_mask", "T_mask")
FIELDS = PLANES + ("adj", "tree_pos", "triplet")
# what each use_pegen mode reads of a batch (CSATrans.process_data builds nothing more from a parents-only batch)
FIELDS_OF_MODE = {"pegen": PLANES, "laplacian": ("adj",), "sequential": (), "treepos": ("tree_pos",),
                  "triplet": ("triplet",)}
_MALFORMED = "parent ids must precede their children (pre-order)"  # csa_ast_relations' message


def _stream(device):
    return _vp(torch.cuda.current_stream(device).cuda_stream)


def malformed(parents, num_node):
    """(B,) bool: which trees break the builders' contract parent[0] < 0, 0 <= parent[v] < v for 0 < v < n (numpy)."""
    parents = np.asarray(parents)
    B, N = parents.shape
    n = np.clip(np.asarray(num_node).reshape(B).astype(np.int64), 0, N)
    v = np.arange(N)[None, :]
    p = parents.astype(np.int64)
    wrong = np.where(v == 0, p >= 0, (p < 0) | (p >= v)) & (v < n[:, None])
    return wrong.any(1)


def ast_batch_host(parents, num_node, max_size=None, fields=PLANES, check=False):
    """The fallback: data.relation_planes (the native host builder) and the numpy builders of data.py, on the host.
    A malformed tree raises under check=True and is built as the empty tree, status 1, otherwise. Synchronises when
    parents is on a device; the fields come back on parents' device."""
    dev = parents.device
    par = parents.detach().cpu().numpy().astype(np.int32)
    B, N = par.shape
    if max_size is not None and max_size != N:
        raise ValueError("ast_batch: max_size must equal parents.shape[1]")
    given = np.clip(torch.as_tensor(num_node).detach().cpu().numpy().reshape(B).astype(np.int64), 0, N)
    bad = malformed(par, given)
    if check and bad.any():
        raise CsaError(f"ast_batch: trees {[int(i) for i in np.nonzero(bad)[0]]}: {_MALFORMED}")
    nn_ = np.where(bad, 0, given)
    out = SimpleNamespace(num_node=torch.as_tensor(given.astype(np.int32)).to(dev),
                          status=torch.as_tensor(bad.astype(np.int32)).to(dev))
    want = [f for f in PLANES if f in fields]
    if want:
        built = dict(zip(PLANES, _data.relation_planes(par, nn_, N)))
        if "L" in fields and "T" in fields:
            out.rel = torch.as_tensor(np.stack([built["L"], built["T"]], 1)).to(dev)
            out.L, out.T = out.rel[:, 0], out.rel[:, 1]
        if "L_mask" in fields and "T_mask" in fields:
            out.rel_mask = torch.as_tensor(np.stack([built["L_mask"], built["T_mask"]], 1).view(np.uint8)).to(dev)
            out.L_mask, out.T_mask = out.rel_mask[:, 0].view(torch.bool), out.rel_mask[:, 1].view(torch.bool)
        for f in want:
            if not hasattr(out, f):
                setattr(out, f, torch.as_tensor(built[f]).to(dev))
    pars = [par[b, :int(nn_[b])].astype(np.int64) for b in range(B)]
    if "adj" in fields:
        out.adj = torch.as_tensor(np.stack([_data.adjacency(p, N) for p in pars])).to(dev)
    if "tree_pos" in fields:
        out.tree_pos = torch.as_tensor(np.stack([_data.tree_positions(p, N) for p in pars])).to(dev)
    if "triplet" in fields:
        out.triplet = torch.as_tensor(np.stack([_data.triplet_ids(p, N) for p in pars])).to(dev)
    return out


def ast_batch(parents, num_node, max_size=None, fields=PLANES, backend="auto", check=False):
    """The structural fields of a batch of ASTs: parents (B, N) integer tensor (parent[0] = -1, 0 <= parent[v] < v: any
    topological numbering, pre-order included; entries beyond num_node are ignored), num_node (B,) -> a namespace with
    the requested `fields` among

      L, T            (B, N, N) uint8   clamp(raw + 75, 0, 149) of the ancestor / sibling relation (data.relation_planes)
      L_mask, T_mask  (B, N, N) bool    raw == 0, torch.bool views of 0/1 bytes
      adj             (B, N, N) bool    data.adjacency
      tree_pos        (B, N, 128) fp32  data.tree_positions
      triplet         (B, N) int64      data.triplet_ids

    and num_node (B,) int32 clamped to [0, N] and status (B,) int32, 1 where a tree is malformed (such a tree gets the
    fields of the empty tree: planes 75, masks True, zeros, PAD; num_node is reported as given). When L and T are both
    requested they are views into rel (B, 2, N, N) uint8, the buffer CSE.forward reads, and L_mask / T_mask into the
    bytes of rel_mask (B, 2, N, N) uint8.

    backend: "auto" runs the device kernel for CUDA tensors with a supported N (csa_ast_batch_supported: N <= 3276) and
    the host builders otherwise; "host" forces the builders; "device" raises where the kernel cannot run. check=True
    reads the status words (one sync) and raises CsaError on a malformed tree; the default path has no sync and
    allocates nothing inside the library call."""
    if parents.dim() != 2:
        raise ValueError("ast_batch: parents must be (B, N)")
    if backend not in ("auto", "host", "device"):
        raise ValueError("ast_batch: backend is 'auto', 'host' or 'device'")
    B, N = parents.shape
    if max_size is not None and max_size != N:
        raise ValueError("ast_batch: max_size must equal parents.shape[1]")
    fields = tuple(fields)
    if any(f not in FIELDS for f in fields):
        raise ValueError(f"ast_batch: fields are among {FIELDS}")
    if torch.as_tensor(num_node).numel() != B:
        raise ValueError("ast_batch: num_node must hold one count per AST")
    can = parents.is_cuda and N >= 1 and bool(lib().csa_ast_batch_supported(N))
    if backend == "device" and not can:
        raise CsaError("ast_batch: the device builder needs CUDA tensors and 1 <= N <= 3276 (csa_ast_batch_supported)")
    if backend == "host" or not can:
        return ast_batch_host(parents, num_node, N, fields, check)
    dev = parents.device
    par = parents.to(torch.int32).contiguous()
    nn_ = torch.as_tensor(num_node).to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    out = SimpleNamespace(num_node=nn_.clamp(0, N), status=torch.empty(B, dtype=torch.int32, device=dev))
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
    args = AstBatchArgs(B=B, N=N, parents=par.data_ptr(), num_node=nn_.data_ptr(), status=out.status.data_ptr())
    pair = lambda a, b: a in fields and b in fields
    if pair("L", "T"):
        out.rel = u8(B, 2, N, N)
        out.L, out.T = out.rel[:, 0], out.rel[:, 1]
    if pair("L_mask", "T_mask"):
        out.rel_mask = u8(B, 2, N, N)
        out.L_mask, out.T_mask = out.rel_mask[:, 0], out.rel_mask[:, 1]
    paired = hasattr(out, "rel") or hasattr(out, "rel_mask")
    for f in PLANES:
        if f in fields and not hasattr(out, f):
            # a plane requested without its partner; with the other pair in a (B, 2, N, N) buffer it takes that
            # buffer's batch stride (the four planes share one)
            setattr(out, f, u8(B, 2, N, N)[:, 0] if paired else u8(B, N, N))
    for f in PLANES:
        if f in fields:
            setattr(args, f, getattr(out, f).data_ptr())
    args.plane_sb = 2 * N * N if paired else 0
    if "adj" in fields:
        out.adj = u8(B, N, N)
        args.adj = out.adj.data_ptr()
    if "tree_pos" in fields:
        out.tree_pos = torch.empty(B, N, 128, dtype=torch.float32, device=dev)
        args.tree_pos = out.tree_pos.data_ptr()
    if "triplet" in fields:
        out.triplet = torch.empty(B, N, dtype=torch.int64, device=dev)
        args.triplet = out.triplet.data_ptr()
    with on_device(dev):
        _check(lib().csa_ast_batch(ctypes.byref(args), _stream(dev)), "csa_ast_batch")
    for f in ("L_mask", "T_mask", "adj"):
        if f in fields:
            setattr(out, f, getattr(out, f).view(torch.bool))
    if check and bool((out.status != 0).any()):
        bad = [int(i) for i in torch.nonzero(out.status).reshape(-1)]
        raise CsaError(f"ast_batch: trees {bad}: {_MALFORMED}")
    return out
