"""The log-probability of given tokens under fp32 logits (csrc/csa_score.hip, csa_token_logp_fwd / _bwd): what
teacher-forced scoring keeps of a (rows, V) generator output, one number per row, without the log-probability tensor
that log_softmax + gather materialise and save.

CUDA fp32 logits within csa_token_logp_supported run the kernels on the current stream with no host sync; CPU tensors,
other dtypes and an unsupported V run the same definition as torch ops (token_logp_host)."""
import ctypes

import torch

from ._lib import check, lib, on_device
from .model import PAD


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def scored_mask(target, V, ignore_id):
    """The rows that are scored: the target is not ignore_id and lies in [0, V)."""
    return (target != ignore_id) & (target >= 0) & (target < V)


def token_logp_host(logits, target, ignore_id=PAD):
    """The fallback: log_softmax + gather + masking in torch, on the tensors' device, differentiable. Half-precision
    logits are scored in fp32; fp64 logits stay fp64."""
    V = logits.shape[-1]
    dt = torch.float64 if logits.dtype == torch.float64 else torch.float32
    ok = scored_mask(target, V, ignore_id)
    if V == 0:
        return torch.zeros(target.shape, dtype=dt, device=logits.device)
    t = torch.where(ok, target, torch.zeros_like(target))
    lp = torch.log_softmax(logits, -1, dtype=dt).gather(-1, t.unsqueeze(-1)).squeeze(-1)
    return torch.where(ok, lp, torch.zeros_like(lp))


class _TokenLogp(torch.autograd.Function):
    """z (rows, V) fp32 CUDA, last dim contiguous, row stride >= V; t (rows) int64 contiguous -> (rows) fp32.
    Saved for the backward: z, t and the row statistics lse (rows, 2), 8 bytes per row."""

    @staticmethod
    def forward(ctx, z, t, ignore_id):
        rows, V = z.shape
        ld = z.stride(0) if rows > 1 else max(z.stride(0), V)
        logp = torch.empty(rows, dtype=torch.float32, device=z.device)
        lse = torch.empty(rows, 2, dtype=torch.float32, device=z.device)
        with on_device(z.device):
            check(lib().csa_token_logp_fwd(_p(z), ld, _p(t), rows, V, ignore_id, _p(logp), _p(lse), _stream(z.device)),
                  "csa_token_logp_fwd")
        ctx.save_for_backward(z, t, lse)
        ctx.cfg = (ld, ignore_id)
        return logp

    @staticmethod
    def backward(ctx, g):
        z, t, lse = ctx.saved_tensors
        ld, ignore_id = ctx.cfg
        rows, V = z.shape
        g = g.contiguous()
        dz = torch.empty(rows, V, dtype=torch.float32, device=z.device)
        with on_device(z.device):
            check(lib().csa_token_logp_bwd(_p(g), _p(z), ld, _p(t), _p(lse), _p(dz), V, rows, V, ignore_id,
                                           _stream(z.device)), "csa_token_logp_bwd")
        return dz, None, None


def _rows(logits):
    """(..., V) -> a (rows, V) view with a contiguous last dim and one row stride of at least V; a copy only where no
    such view exists (a strided last dim, leading dims that do not collapse, overlapping rows)."""
    V = logits.shape[-1]
    z = logits.reshape(-1, V)
    if (V > 1 and z.stride(1) != 1) or (z.shape[0] > 1 and z.stride(0) < V) or z.data_ptr() % 4:
        z = z.contiguous()
    return z


def token_logp(logits, target, ignore_id=PAD):
    """logits (..., V), target (...) int64 -> (...) fp32: log_softmax(logits)[target] per row, 0 where the target is
    ignore_id or lies outside [0, V). A true log-softmax (max-subtracted; a probability that underflows in fp32 still has
    its finite log-probability), unlike the Generator's log(softmax). Differentiable in logits:
    d logits = g * (onehot(target) - softmax(logits)), zeros in ignored rows whatever g holds there.

    On the GPU the logits are read where they are when their last dim is contiguous and their rows have one stride
    (a column slice of a wider buffer); anything else is copied once. Nothing of size (rows, V) is saved beyond the
    logits themselves. No host sync."""
    if not isinstance(logits, torch.Tensor) or not isinstance(target, torch.Tensor) or logits.dim() < 1:
        raise TypeError("token_logp: logits (..., V) and target (...) must be tensors")
    if target.dtype != torch.int64 or target.shape != logits.shape[:-1]:
        raise ValueError("token_logp: target must be int64 of the logits' shape without its last dim")
    if target.device != logits.device:
        raise ValueError("token_logp: logits and target must be on one device")
    ignore_id = int(ignore_id)
    V = logits.shape[-1]
    if not (logits.is_cuda and logits.dtype == torch.float32 and lib().csa_token_logp_supported(V)):
        return token_logp_host(logits, target, ignore_id)
    if target.numel() == 0:
        return torch.zeros(target.shape, dtype=torch.float32, device=logits.device)
    return _TokenLogp.apply(_rows(logits), target.reshape(-1).contiguous(), ignore_id).view(target.shape)
