"""Full-sequence (teacher-forced) decoder attention (csrc/csa_seqattn.hip, csa_seq_attn_fwd / _bwd):

    out[r, i, h*hd:(h+1)*hd] = sum_j softmax_j(scale * q[r,h,i] . K[kb,h,j] + m(r,h,i,j)) * V[kb,h,j],  kb = r // kv_group

with the causal, PAD and memory masks applied inside the kernel from uint8 rows, the kv_group query rows of an AST
reading one K/V, and their dK / dV summed inside the kernel in a fixed order. What the decode step has for one query
position (decode_ops.decode_attention, kv_group), for all T positions at once and differentiable.

fp32 CUDA tensors within csa_seq_attn_supported run the kernels on the current stream with no host sync, allocating
the output, lse (R, H, T), and in the backward the gradients and an (R, H, T) workspace; CPU tensors, other dtypes and
unsupported shapes run the same definition as torch ops (seq_attention_host), differentiable."""
import ctypes

import torch
import torch.nn.functional as F

from ._lib import SeqAttnArgs, SeqAttnBwdArgs, check, lib, on_device
from .ops import packed_grads, packed_qkv

MASK_MODES = ("own", "reference")


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def masked_keys(R, H, T, S, key_mask, causal, mask_mode, kv_group, device):
    """The mask rule written out: (R, H, T | 1, S) bool, True = key j is masked for query i of (r, h), or None when
    nothing is. causal: j > i. key_mask (rows, >= S), non-zero = masked: row r // kv_group ("own") or row
    (r * H + h) % R ("reference")."""
    dead = None
    if key_mask is not None:
        km = key_mask[:, :S] != 0
        r = torch.arange(R, device=device)
        if mask_mode == "own":
            dead = km[r // kv_group].view(R, 1, 1, S)
        else:
            h = torch.arange(H, device=device)
            dead = km[(r[:, None] * H + h[None, :]) % R].view(R, H, 1, S)
    if causal:
        future = torch.triu(torch.ones(T, S, dtype=torch.bool, device=device), diagonal=1).view(1, 1, T, S)
        dead = future if dead is None else dead | future
    return dead


def seq_attention_host(q, k, v, key_mask=None, causal=False, mask_mode="own", kv_group=1, scale=None):
    """The definition in torch ops on the tensors' device, differentiable: masked softmax on expanded K/V."""
    R, H, T, hd = q.shape
    S = k.shape[2]
    scale = float(hd) ** -0.5 if scale is None else scale
    if kv_group > 1:
        k, v = k.repeat_interleave(kv_group, 0), v.repeat_interleave(kv_group, 0)
    s = (q @ k.transpose(-1, -2)) * scale
    dead = masked_keys(R, H, T, S, key_mask, causal, mask_mode, kv_group, q.device)
    if dead is not None:
        s = s.masked_fill(dead, float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(R, T, H * hd)


def seq_attention_sdpa(q, k, v, key_mask=None, causal=False, mask_mode="own", kv_group=1, dropout_p=0.0):
    """The same attention on F.scaled_dot_product_attention with an explicit additive -inf mask and expanded K/V: the
    path the decoder's forward() takes, attention dropout included."""
    R, H, T, hd = q.shape
    S = k.shape[2]
    if kv_group > 1:
        k, v = k.repeat_interleave(kv_group, 0), v.repeat_interleave(kv_group, 0)
    dead = masked_keys(R, H, T, S, key_mask, causal, mask_mode, kv_group, q.device)
    m = None if dead is None else torch.zeros(dead.shape, dtype=q.dtype, device=q.device).masked_fill_(dead, float("-inf"))
    return F.scaled_dot_product_attention(q, k, v, m, dropout_p).transpose(1, 2).reshape(R, T, H * hd)


def _packed_kv(k, v):
    """k, v are the two head-major views of one packed (B, S, 2, H, hd) projection (split_heads_kv)."""
    if k.shape != v.shape or k.stride() != v.stride() or k.dim() != 4 or k.dtype != torch.float32:
        return False
    B, H, S, d = k.shape
    return (k.stride() == (S * 2 * H * d, d, 2 * H * d, 1)
            and k.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()
            and v.storage_offset() == k.storage_offset() + H * d)


class _SplitHeadsKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        return y[:, :, 0].transpose(1, 2), y[:, :, 1].transpose(1, 2)

    @staticmethod
    def backward(ctx, dk, dv):
        ref = dk if dk is not None else dv
        B, H, S, d = ref.shape
        if dk is not None and dv is not None and _packed_kv(dk, dv):  # the kernel wrote the packed layout already
            return dk.as_strided((B, S, 2, H, d), (S * 2 * H * d, 2 * H * d, H * d, d, 1), dk.storage_offset())
        out = torch.empty(B, S, 2, H, d, device=ref.device, dtype=ref.dtype)
        for i, g in enumerate((dk, dv)):
            if g is None:
                out[:, :, i].zero_()
            else:
                out[:, :, i].transpose(1, 2).copy_(g)
        return out


def split_heads_kv(y):
    """A packed memory projection (B, S, 2, H, hd) -> K, V as strided (B, H, S, hd) views, as unbind(2) + transpose(1, 2)
    gives them; the backward hands a packed gradient over as it is when seq_attention wrote dk / dv into one (no stack)."""
    if y.dim() != 5 or y.shape[2] != 2 or not y.is_contiguous():
        return tuple(t.transpose(1, 2) for t in y.unbind(2))
    return _SplitHeadsKV.apply(y)


def _operand(t):
    """t as a tensor the kernels take in place: hd contiguous, strides multiples of 4 elements, 16-byte aligned; a
    contiguous copy otherwise."""
    if t.stride(-1) != 1 or any(s % 4 for s in t.stride()[:-1]) or t.data_ptr() % 16:
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    return t


class _SeqAttn(torch.autograd.Function):
    """q (R, H, T, hd), k / v (R / G, H, S, hd) fp32 CUDA kernel operands, mask (rows, >= S) uint8 or None.
    Saved for the backward: q, k, v, the mask, out and lse (R, H, T)."""

    @staticmethod
    def forward(ctx, q, k, v, mask, causal, mode, G, scale):
        R, H, T, hd = q.shape
        S = k.shape[2]
        out = torch.empty(R, T, H * hd, dtype=torch.float32, device=q.device)
        lse = torch.empty(R, H, T, dtype=torch.float32, device=q.device)
        a = _SeqAttn._args(q, k, v, mask, causal, mode, G, scale, out, lse)
        with on_device(q.device):
            check(lib().csa_seq_attn_fwd(ctypes.byref(a), _stream(q.device)), "csa_seq_attn_fwd")
        ctx.save_for_backward(q, k, v, mask, out, lse)
        ctx.cfg = (causal, mode, G, scale)
        return out

    @staticmethod
    def _args(q, k, v, mask, causal, mode, G, scale, out, lse):
        R, H, T, hd = q.shape
        return SeqAttnArgs(R=R, H=H, T=T, S=k.shape[2], hd=hd, kv_group=G,
                           q=_p(q), q_sr=q.stride(0), q_sh=q.stride(1), q_st=q.stride(2),
                           k=_p(k), k_sb=k.stride(0), k_sh=k.stride(1), k_sn=k.stride(2),
                           v=_p(v), v_sb=v.stride(0), v_sh=v.stride(1), v_sn=v.stride(2),
                           mask=_p(mask), mask_ld=mask.stride(0) if mask is not None else 0,
                           mask_mode=mode, causal=int(causal), scale=scale, out=_p(out), lse=_p(lse))

    @staticmethod
    def backward(ctx, g):
        q, k, v, mask, out, lse = ctx.saved_tensors
        causal, mode, G, scale = ctx.cfg
        R, H, T, hd = q.shape
        B, S = k.shape[0], k.shape[2]
        dev = q.device
        g = g.contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        new = lambda n, rows: torch.empty(n, rows, H, hd, dtype=torch.float32, device=dev).transpose(1, 2)
        if packed_qkv(q, k, v):  # self-attention on one packed projection: one packed gradient (glue.split_heads3)
            _, (dq, dk, dv) = packed_grads(R, H, T, hd, dev)
        else:
            dq = new(R, T)
            if _packed_kv(k, v):  # the two planes of a memory projection (split_heads_kv)
                pk = torch.empty(B, S, 2, H, hd, dtype=torch.float32, device=dev)
                dk, dv = pk[:, :, 0].transpose(1, 2), pk[:, :, 1].transpose(1, 2)
            else:
                dk, dv = new(B, S), new(B, S)
        L = lib()
        ws = torch.empty(max(1, L.csa_seq_attn_bwd_workspace_bytes(R, H, T)), dtype=torch.uint8, device=dev)
        a = _SeqAttn._args(q, k, v, mask, causal, mode, G, scale, out, lse)
        b = SeqAttnBwdArgs(fwd=ctypes.pointer(a), dout=_p(g),
                           dq=_p(dq), dq_sr=dq.stride(0), dq_sh=dq.stride(1), dq_st=dq.stride(2),
                           dk=_p(dk), dk_sb=dk.stride(0), dk_sh=dk.stride(1), dk_sn=dk.stride(2),
                           dv=_p(dv), dv_sb=dv.stride(0), dv_sh=dv.stride(1), dv_sn=dv.stride(2), workspace=_p(ws))
        with on_device(dev):
            check(L.csa_seq_attn_bwd(ctypes.byref(b), _stream(dev)), "csa_seq_attn_bwd")
        return dq, dk, dv, None, None, None, None, None


def seq_attention(q, k, v, key_mask=None, causal=False, mask_mode="own", kv_group=1):
    """q (R, H, T, hd), k / v (R / kv_group, H, S, hd) -> (R, T, H*hd) contiguous, batch-first (what out_proj reads),
    scale hd^-0.5. q, k, v may be the strided views of a packed (B, T, 3, H, hd) or (B, S, 2, H, hd) projection
    (glue.split_heads3, split_heads_kv): the kernels read them in place and write dq / dk / dv into one packed gradient.

    A key j is masked (-inf) for query i of row r, head h when causal and j > i (causal needs S == T and
    kv_group == 1), or when key_mask (rows, >= S) uint8 / bool holds a non-zero byte at column j of row
      "own"        r // kv_group: a (B, S) memory mask, or with kv_group == 1 a row's own PAD columns;
      "reference"  (r * H + h) % R: the reference's head-repeated target mask (DecodeCache.head_pad's rule).
    A query row with every key masked gives NaN in out, as SDPA does; its gradients are unspecified.
    Differentiable in q, k, v; dk / dv sum over the kv_group rows of an AST inside the kernel, in a fixed order:
    bitwise reproducible. No host sync."""
    if not all(isinstance(t, torch.Tensor) and t.dim() == 4 for t in (q, k, v)):
        raise TypeError("seq_attention: q (R, H, T, hd) and k, v (R / kv_group, H, S, hd) must be tensors")
    if mask_mode not in MASK_MODES:
        raise ValueError(f"seq_attention: mask_mode must be one of {MASK_MODES}")
    R, H, T, hd = q.shape
    G = int(kv_group)
    if G < 1 or R % G:
        raise ValueError("seq_attention: kv_group must be positive and divide the rows of q")
    if k.shape != v.shape or k.shape[0] * G != R or k.shape[1] != H or k.shape[3] != hd:
        raise ValueError("seq_attention: k and v must be (R / kv_group, H, S, hd)")
    S = k.shape[2]
    if T < 1 or S < 1:
        raise ValueError("seq_attention: T and S must be at least 1")
    if causal and (S != T or G != 1):
        raise ValueError("seq_attention: causal needs S == T and kv_group == 1")
    if k.dtype != q.dtype or v.dtype != q.dtype or k.device != q.device or v.device != q.device:
        raise ValueError("seq_attention: q, k, v must share dtype and device")
    if key_mask is not None:
        rows = R if mask_mode == "reference" else R // G
        if (key_mask.dtype not in (torch.uint8, torch.bool) or key_mask.dim() != 2 or key_mask.shape[0] != rows
                or key_mask.shape[1] < S or key_mask.device != q.device):
            raise ValueError(f"seq_attention: key_mask must be ({rows}, >= S) uint8 or bool on q's device")
    if not (q.is_cuda and q.dtype == torch.float32 and lib().csa_seq_attn_supported(hd, T, S)):
        return seq_attention_host(q, k, v, key_mask, bool(causal), mask_mode, G)
    mask = None
    if key_mask is not None:
        mask = key_mask if key_mask.stride(1) == 1 and key_mask.stride(0) >= S else key_mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return _SeqAttn.apply(_operand(q), _operand(k), _operand(v), mask, bool(causal), MASK_MODES.index(mask_mode), G,
                          float(hd) ** -0.5)
