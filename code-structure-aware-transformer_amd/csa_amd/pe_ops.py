"""The structure encodings of the use_pegen ablations on the device (csrc/csa_pe.hip).

tree_pos_encode: TreePositionalEncodings.forward (module/csa_trans.py:41-64) as one kernel per direction; only
the parameter p has a gradient. CPU tensors take the reference's torch expressions.

lap_pe: the Laplacian eigenvectors of a batch of ASTs (module/base_seq2seq.py:12-36,70-82) from one kernel, one
workgroup per AST, instead of a device-to-host copy and a LAPACK eigh per AST per forward call. CPU tensors, shapes
the kernel does not support and backend="host" take torch.linalg.eigh per AST on the host with the same sign rule.
"""
import ctypes
from collections import namedtuple

import torch

from ._lib import CsaError, LapPeArgs, lib, on_device
from ._lib import check as _check

_vp = ctypes.c_void_p


def _stream(device):
    return _vp(torch.cuda.current_stream(device).cuda_stream)


def tree_weights(p, depth, width, d_model):
    """TreePositionalEncodings.build_weights (module/csa_trans.py:41-48): (depth * width, n_feat)."""
    n_feat = p.numel()
    t = torch.tanh(p)
    tiled = t.reshape((1, 1, -1)).repeat(depth, width, 1)
    depths = torch.arange(depth, dtype=p.dtype, device=p.device).reshape(-1, 1, 1).repeat(1, width, n_feat)
    norm = torch.sqrt((1 - torch.square(t)) * d_model / 2)
    return (torch.pow(tiled, depths) * norm).reshape(depth * width, n_feat)


def tree_pos_reference(pos, p, depth, width, d_model):
    """TreePositionalEncodings.forward in the reference's torch expressions (treeify_positions, :50-55)."""
    out = pos.unsqueeze(-1) * tree_weights(p, depth, width, d_model)
    return out.reshape(out.shape[:-2] + (depth * width * p.numel(),))


class _TreePosFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, p, depth, width, d_model):
        pos2 = pos.reshape(-1, depth * width).contiguous()
        pc = p.contiguous()
        rows, F = pos2.shape[0], pc.numel()
        out = torch.empty(rows, depth * width * F, dtype=torch.float32, device=pos.device)
        with on_device(pos.device):
            _check(lib().csa_tree_pos_fwd(_vp(pos2.data_ptr()), _vp(pc.data_ptr()), _vp(out.data_ptr()), rows, depth,
                                          width, F, float(d_model), _stream(pos.device)), "csa_tree_pos_fwd")
        ctx.save_for_backward(pos2, pc)
        ctx.dims = (depth, width, float(d_model))
        return out.view(pos.shape[:-1] + (depth * width * F,))

    @staticmethod
    def backward(ctx, g):
        pos2, pc = ctx.saved_tensors
        depth, width, d_model = ctx.dims
        rows, F = pos2.shape[0], pc.numel()
        g2 = g.reshape(rows, depth * width * F)
        if not g2.is_contiguous() or g2.dtype != torch.float32:
            g2 = g2.float().contiguous()
        L = lib()
        dp = torch.empty(F, dtype=torch.float32, device=pc.device)
        ws = torch.empty(max(8, L.csa_tree_pos_bwd_workspace_bytes(rows, depth, width, F)), dtype=torch.uint8,
                         device=pc.device)
        with on_device(pc.device):
            _check(L.csa_tree_pos_bwd(_vp(pos2.data_ptr()), _vp(pc.data_ptr()), _vp(g2.data_ptr()), _vp(dp.data_ptr()),
                                      rows, depth, width, F, d_model, _vp(ws.data_ptr()), _stream(pc.device)),
                   "csa_tree_pos_bwd")
        return None, dp.view(pc.shape), None, None, None


def tree_pos_encode(pos, p, depth=16, width=8, d_model=None):
    """pos (..., depth * width), p (n_feat,) -> (..., depth * width * n_feat); d_model defaults to the output
    width. CUDA fp32 runs csa_tree_pos_fwd / csa_tree_pos_bwd (a shape they do not support is an error, not a
    fallback); CPU tensors take the reference's torch expressions."""
    if d_model is None:
        d_model = depth * width * p.numel()
    if pos.shape[-1] != depth * width:
        raise ValueError(f"tree_pos_encode: the last dim of pos must be depth * width = {depth * width}")
    if not pos.is_cuda:
        return tree_pos_reference(pos, p, depth, width, d_model)
    if pos.dtype != torch.float32 or p.dtype != torch.float32 or p.device != pos.device:
        raise CsaError("tree_pos_encode: fp32 pos and p on one device")
    if not lib().csa_tree_pos_supported(depth, width, p.numel()):
        raise CsaError("tree_pos_encode: needs depth <= 64 and depth * width * n_feat <= 1024 (csa_tree_pos_supported)")
    return _TreePosFn.apply(pos, p, depth, width, d_model)


LapPE = namedtuple("LapPE", "pe eigenvalues status sweeps")
LapPE.__doc__ = """lap_pe's result: pe (B, N, pegen_dim) fp32, eigenvalues (B, N) fp32 (zeros beyond num_node),
status (B,) int32 (0, or 1 where the device solver reached its sweep cap) and sweeps (B,) int32 (Jacobi sweeps run;
0 on the host)."""


def _fix_signs(vec):
    """Flip each column so that its largest-magnitude entry (the first on ties) is positive."""
    idx = vec.abs().argmax(dim=0)  # the first index among equal maxima
    sgn = torch.where(vec.gather(0, idx[None])[0] < 0, -1.0, 1.0).to(vec.dtype)
    return vec * sgn[None]


def lap_pe_host(adj, num_node, pegen_dim):
    """The fallback: per AST, L = I - D^-1/2 A D^-1/2 of A = adj[b, :n, :n] != 0 on the host (D^-1/2 A D^-1/2 in
    fp32, L and torch.linalg.eigh in fp64, as the reference's numpy does; ascending eigenvalues), with lap_pe's sign
    rule, returned as fp32. Synchronises when adj is on a device."""
    B, N = adj.shape[0], adj.shape[1]
    if pegen_dim < N:
        raise ValueError("lap_pe: pegen_dim must be at least N")
    a = adj.detach().cpu() != 0
    nn_ = [int(v) for v in torch.as_tensor(num_node).detach().cpu().reshape(-1)]
    pe = torch.zeros(B, N, pegen_dim, dtype=torch.float32)
    ev = torch.zeros(B, N, dtype=torch.float32)
    for b in range(B):
        n = min(max(nn_[b], 0), N)
        if n == 0:
            continue
        A = a[b, :n, :n].to(torch.float32)
        dinv = A.sum(1).clamp(min=1).pow(-0.5)
        Lm = torch.eye(n, dtype=torch.float64) - (dinv[:, None] * A * dinv[None, :]).double()  # as the reference
        val, vec = torch.linalg.eigh(Lm)
        pe[b, :n, :n] = _fix_signs(vec.float())
        ev[b, :n] = val.float()
    dev = adj.device
    z = torch.zeros(B, dtype=torch.int32, device=dev)
    return LapPE(pe.to(dev), ev.to(dev), z, z.clone())


def lap_pe(adj, num_node, pegen_dim, backend="auto", check=False):
    """Laplacian positional encodings of a batch: adj (B, N, N) bool or uint8 (non-zero = edge, symmetric), num_node
    (B,) -> LapPE. Per AST with n = num_node[b], pe[b, :n, :n] holds the eigenvectors of L = I - D^-1/2 A D^-1/2 as
    columns in ascending order of eigenvalue, A = adj[b, :n, :n] (anything outside that block is ignored, as the
    reference's slice does), D the row sums of A clipped below at 1; zeros everywhere else. Each eigenvector has its
    largest-magnitude entry (the first on ties) positive; inside the eigenspace of a repeated eigenvalue the basis
    is any orthonormal one.

    backend: "auto" runs the device kernel for CUDA tensors it supports (csa_lap_pe_supported: N <= pegen_dim and
    N <= 201) and the host fallback otherwise; "host" forces the fallback; "device" raises where the kernel cannot
    run. check=True reads the status words (one sync) and raises on a non-zero one; the default path has no sync."""
    if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
        raise ValueError("lap_pe: adj must be (B, N, N)")
    if adj.dtype not in (torch.bool, torch.uint8):
        raise ValueError("lap_pe: adj must be bool or uint8")
    if backend not in ("auto", "host", "device"):
        raise ValueError("lap_pe: backend is 'auto', 'host' or 'device'")
    B, N = adj.shape[0], adj.shape[1]
    if num_node.numel() != B:
        raise ValueError("lap_pe: num_node must hold one count per AST")
    if pegen_dim < N:
        raise ValueError("lap_pe: pegen_dim must be at least N")
    can = adj.is_cuda and N >= 1 and bool(lib().csa_lap_pe_supported(N, pegen_dim))
    if backend == "device" and not can:
        raise CsaError("lap_pe: the device solver needs CUDA tensors, N <= pegen_dim and N <= 201 (csa_lap_pe_supported)")
    if backend == "host" or not can:
        return lap_pe_host(adj, num_node, pegen_dim)
    dev = adj.device
    a8 = adj.contiguous().view(torch.uint8)
    nn_ = num_node.to(device=dev, dtype=torch.int32).contiguous()
    pe = torch.empty(B, N, pegen_dim, dtype=torch.float32, device=dev)
    ev = torch.empty(B, N, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    sweeps = torch.empty(B, dtype=torch.int32, device=dev)
    args = LapPeArgs(B=B, N=N, pegen_dim=pegen_dim, adj=a8.data_ptr(), num_node=nn_.data_ptr(), pe=pe.data_ptr(),
                     eigenvalues=ev.data_ptr(), status=status.data_ptr(), sweeps=sweeps.data_ptr())
    with on_device(dev):
        _check(lib().csa_lap_pe(ctypes.byref(args), _stream(dev)), "csa_lap_pe")
    if check and bool((status != 0).any()):
        bad = [int(i) for i in torch.nonzero(status).reshape(-1)]
        raise CsaError(f"lap_pe: the Jacobi sweep cap was reached before convergence for ASTs {bad}")
    return LapPE(pe, ev, status, sweeps)
