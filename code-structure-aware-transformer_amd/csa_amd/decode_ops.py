"""One KV-cached decode step's non-GEMM ops (csrc/csa_decode.hip, ABI v10): single-query attention against a
K/V cache or a projected memory (csa_decode_attn) and the row argmax of the last-position logits written in
place into the token buffer (csa_argmax_rows). Inference only: no autograd.

Device-stepped calls (the captured decode step of CachedGreedyGenerator(graph=True)): where the step index is given as a
1-element int32 tensor instead of an int, the HIP kernels read it on the device (csa_decode_attn_step,
csa_argmax_rows_step, csa_decode_embed) and the host never learns its value, so the same launch serves every step.

fp32 CUDA tensors with a supported head dim run the HIP kernels; CPU tensors, other dtypes or an unsupported
head dim run the same cached algorithm on F.scaled_dot_product_attention / torch.max over the same views."""
import ctypes

import torch
import torch.nn.functional as F

from ._lib import DecodeAttnArgs, check, lib, on_device
from .ops import _stream


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _hip_ok(q, hd):
    return q.is_cuda and q.dtype == torch.float32 and bool(lib().csa_decode_attn_supported(hd))


def _is_step(t):
    return isinstance(t, torch.Tensor)


def _check_step(t, device, what):
    if t.dtype != torch.int32 or t.numel() != 1 or t.device != device:
        raise ValueError(f"{what}: the device step must be a 1-element int32 tensor on the tensors' device")


def _decode_attention_hip(q, K, V, length, key_mask, k_new, v_new, t, scale, out=None):
    B, H, hd = q.shape
    if out is None:
        out = torch.empty(B, H * hd, device=q.device, dtype=torch.float32)
    step = _is_step(t)
    a = DecodeAttnArgs(B=B, H=H, hd=hd, len=length, t=t if k_new is not None and not step else 0,
                       q=_ptr(q), q_sb=q.stride(0), q_sh=q.stride(1),
                       K=_ptr(K), k_sb=K.stride(0), k_sh=K.stride(1), k_sn=K.stride(2),
                       V=_ptr(V), v_sb=V.stride(0), v_sh=V.stride(1), v_sn=V.stride(2),
                       mask=_ptr(key_mask), mask_sb=key_mask.stride(0) if key_mask is not None else 0,
                       mask_sh=key_mask.stride(1) if key_mask is not None and key_mask.dim() == 3 else 0,
                       scale=scale, out=_ptr(out))
    if k_new is not None:
        a.k_new, a.kn_sb, a.kn_sh = _ptr(k_new), k_new.stride(0), k_new.stride(1)
        a.v_new, a.vn_sb, a.vn_sh = _ptr(v_new), v_new.stride(0), v_new.stride(1)
    with on_device(q.device):
        if step:  # length is the capacity; the kernel reads t and attends to t + 1 keys
            check(lib().csa_decode_attn_step(ctypes.byref(a), _ptr(t), _stream(q.device)), "csa_decode_attn_step")
        else:
            check(lib().csa_decode_attn(ctypes.byref(a), _stream(q.device)), "csa_decode_attn")
    return out


def _decode_attention_ref(q, K, V, length, key_mask, k_new, v_new, t, scale, out=None):
    B, H, hd = q.shape
    if _is_step(t):  # the host reads the counter: not for a captured graph
        t, cap = int(t.item()), length
        if not 0 <= t < cap:
            raise ValueError(f"decode_attention: step {t} outside the capacity {cap}")
        length = t + 1
    if k_new is not None:
        K[:, :, t] = k_new
        V[:, :, t] = v_new
    m = None
    if key_mask is not None:
        km = key_mask[..., :length].ne(0).view(B, -1, 1, length)  # (B, 1 | H, 1, length)
        m = torch.zeros(km.shape, dtype=q.dtype, device=q.device).masked_fill_(km, float("-inf"))
    o = F.scaled_dot_product_attention(q.unsqueeze(2), K[:, :, :length], V[:, :, :length], m, scale=scale)
    o = o.reshape(B, H * hd)
    return o if out is None else out.copy_(o)


def decode_attention(q, K, V, length=None, key_mask=None, k_new=None, v_new=None, t=None, scale=None, out=None):
    """Single-query attention of one decode step.

    q (B,H,hd); K, V (B,H,>=length,hd) views (any batch / head / key strides, hd contiguous); key_mask optional
    (B,>=length) uint8, or (B,H,>=length) for a per-head mask, last dim contiguous, non-zero = masked key. Returns
    (B, H*hd) contiguous.
    Append mode (k_new, v_new (B,H,hd) and t given): the rows are stored into K[:, :, t] / V[:, :, t] and serve
    as key t; length is t + 1.
    Device-stepped append (t a 1-element int32 tensor on q's device): the HIP kernel reads the step itself and
    attends to t + 1 keys; length is then the CAPACITY (default K.shape[2]: the rows K, V and key_mask hold), and a
    step outside [0, capacity) stores nothing, neither the cache row nor the output. Off the HIP path the step is read
    on the host (t.item()) and the int path runs.
    out: optional (B, H*hd) fp32 contiguous tensor to receive the result."""
    B, H, hd = q.shape
    if (k_new is None) != (v_new is None) or (k_new is not None and t is None):
        raise ValueError("decode_attention: k_new, v_new and t go together")
    if _is_step(t):
        if k_new is None:
            raise ValueError("decode_attention: a device step needs k_new and v_new (append mode)")
        _check_step(t, q.device, "decode_attention")
        length = K.shape[2] if length is None else length
        if V.shape[2] < length:
            raise ValueError("decode_attention: V holds fewer rows than the capacity")
    elif k_new is not None:
        if length is not None and length != t + 1:
            raise ValueError("decode_attention: append mode needs length == t + 1")
        length = t + 1
    elif length is None:
        length = K.shape[2]
    if not 1 <= length <= K.shape[2] or (key_mask is not None and key_mask.shape[-1] < length):
        raise ValueError("decode_attention: length outside the keys / mask given")
    if key_mask is not None and (key_mask.dtype != torch.uint8 or key_mask.stride(-1) != 1
                                 or key_mask.shape[:-1] not in ((B,), (B, H))):
        raise ValueError("decode_attention: key_mask must be (B, L) or (B, H, L) uint8 with a contiguous last dim")
    scale = float(hd) ** -0.5 if scale is None else float(scale)
    ts = [x for x in (q, K, V, k_new, v_new) if x is not None]
    if any(x.stride(-1) != 1 for x in ts):
        raise ValueError("decode_attention: the head dim must be contiguous")
    if out is not None and (out.shape != (B, H * hd) or out.dtype != q.dtype or out.device != q.device
                            or not out.is_contiguous()):
        raise ValueError("decode_attention: out must be (B, H*hd) contiguous, of q's dtype and device")
    extra = () if out is None else (out,)
    if _hip_ok(q, hd) and all(x.is_cuda and x.dtype == torch.float32 for x in ts):
        return _decode_attention_hip(q, K, V, length, key_mask, k_new, v_new, t, scale, *extra)
    return _decode_attention_ref(q, K, V, length, key_mask, k_new, v_new, t, scale, *extra)


def _argmax_rows_hip(x, out, is_pad, pad_id, maxval):
    rows, V = x.shape
    with on_device(x.device):
        check(lib().csa_argmax_rows(_ptr(x), rows, V, _ptr(out), out.stride(0), _ptr(is_pad),
                                    is_pad.stride(0) if is_pad is not None else 0, pad_id, _ptr(maxval),
                                    _stream(x.device)), "csa_argmax_rows")


def _argmax_rows_ref(x, out, is_pad, pad_id, maxval):
    v, i = torch.max(x, dim=1)
    out.copy_(i)
    if is_pad is not None:
        is_pad.copy_(i == pad_id)
    if maxval is not None:
        maxval.copy_(v)


def _head_view(head_pad, rows):
    """The (H, rows, T) view of a contiguous (rows, H, T) per-head mask in which the decoder key-pads its heads."""
    return head_pad.view(head_pad.shape[1], rows, head_pad.shape[2])


def _argmax_rows_step(x, ys, pad, pad_id, t_dev, head_pad):
    rows, V = x.shape
    T = ys.shape[1] if ys.dim() == 2 else -1
    if (ys.dtype != torch.int64 or ys.dim() != 2 or ys.shape[0] != rows or ys.stride(1) != 1 or ys.device != x.device
            or (pad is not None and (pad.dtype != torch.uint8 or pad.shape != (rows, T) or pad.stride(1) != 1
                                     or pad.device != x.device))
            or (head_pad is not None and (head_pad.dtype != torch.uint8 or head_pad.dim() != 3
                                          or head_pad.shape[0] != rows or head_pad.shape[2] != T
                                          or not head_pad.is_contiguous() or head_pad.device != x.device))):
        raise ValueError("argmax_rows: with t_dev, out is the (rows, T) int64 token buffer, is_pad (rows, T) uint8, both "
                         "with a contiguous last dim, and head_pad (rows, H, T) uint8 contiguous")
    _check_step(t_dev, x.device, "argmax_rows")
    if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and V >= 1:
        with on_device(x.device):
            check(lib().csa_argmax_rows_step(_ptr(x), rows, V, _ptr(ys), ys.stride(0), T, _ptr(pad),
                                             pad.stride(0) if pad is not None else 0, _ptr(head_pad),
                                             head_pad.shape[1] if head_pad is not None else 0, pad_id, _ptr(t_dev),
                                             _stream(x.device)), "csa_argmax_rows_step")
        return ys
    col = int(t_dev.item()) + 1  # the host reads the counter: not for a captured graph
    if not 1 <= col < T:
        raise ValueError(f"argmax_rows: column {col} outside [1, {T})")
    _argmax_rows_ref(x, ys[:, col], None if pad is None else pad[:, col], pad_id, None)
    if head_pad is not None:
        _head_view(head_pad, rows)[:, :, col] = ys[:, col] == pad_id
    return ys


def argmax_rows(x, out=None, is_pad=None, pad_id=0, maxval=None, t_dev=None, head_pad=None):
    """Row argmax of x (rows, V) into `out` (rows,) int64, which may be a strided column such as ys[:, t+1];
    ties go to the lowest index. Optionally is_pad (rows,) uint8 (strided) receives (index == pad_id) and maxval
    (rows,) fp32 contiguous the row maximum. Returns out.
    Device-stepped (t_dev a 1-element int32 tensor): out is the whole (rows, T) token buffer and is_pad the whole
    (rows, T) mask; the kernel reads t and writes column t + 1 of both and, when head_pad (rows, H, T) is given, the
    same byte into head_pad.view(H, rows, T)[:, r, t + 1], the column BaseDecoder.step would copy from is_pad at the
    top of step t + 1. A column outside [1, T) stores nothing."""
    if t_dev is not None:
        if out is None or maxval is not None:
            raise ValueError("argmax_rows: with t_dev, out is required and maxval is not available")
        return _argmax_rows_step(x, out, is_pad, pad_id, t_dev, head_pad)
    if head_pad is not None:
        raise ValueError("argmax_rows: head_pad goes with t_dev")
    rows, V = x.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=x.device)
    if out.dtype != torch.int64 or out.shape != (rows,) or (is_pad is not None and (
            is_pad.dtype != torch.uint8 or is_pad.shape != (rows,))) or (maxval is not None and (
            maxval.dtype != torch.float32 or maxval.shape != (rows,) or not maxval.is_contiguous())):
        raise ValueError("argmax_rows: out (rows,) int64, is_pad (rows,) uint8, maxval (rows,) fp32 contiguous")
    if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and V >= 1:
        _argmax_rows_hip(x, out, is_pad, pad_id, maxval)
    else:
        _argmax_rows_ref(x, out, is_pad, pad_id, maxval)
    return out


def decode_embed(ys, t, emb):
    """Embeddings.step for the position held in the device counter: LayerNorm(W[ys[:, t]] + pe[t]) -> (B, E).

    ys (B, T) int64 token buffer (row stride free, last dim contiguous), t a 1-element int32 tensor, emb a
    csa_amd.model.Embeddings in eval mode (its dropout is the identity). fp32 CUDA parameters with a supported E run
    csa_decode_embed, bitwise the gather + add + csa_layernorm_fwd of Embeddings.step; anything else reads the step on
    the host and runs Embeddings.step itself."""
    if emb.training:
        raise ValueError("decode_embed: inference only (the module is in training mode)")
    _check_step(t, ys.device, "decode_embed")
    if ys.dtype != torch.int64 or ys.dim() != 2 or ys.stride(1) != 1:
        raise ValueError("decode_embed: ys must be (B, T) int64 with a contiguous last dim")
    W, norm = emb.word_embeddings.weight, emb.norm
    pe = emb.pos_emb.pe[0] if emb.pos_emb is not None else None
    B, T = ys.shape
    E = W.shape[1]
    fp32 = [W, norm.weight, norm.bias] + ([pe] if pe is not None else [])
    if (ys.is_cuda and all(p is not None and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in fp32)
            and lib().csa_layernorm_supported(E)):
        x = torch.empty(B, E, device=ys.device, dtype=torch.float32)
        with on_device(ys.device):
            check(lib().csa_decode_embed(_ptr(ys), ys.stride(0), B, T, _ptr(t), _ptr(W), W.shape[0], _ptr(pe),
                                         pe.shape[0] if pe is not None else 0, _ptr(norm.weight), _ptr(norm.bias),
                                         float(norm.eps), _ptr(x), E, _stream(ys.device)), "csa_decode_embed")
        return x
    tt = int(t.item())  # the host reads the counter: not for a captured graph
    if not 0 <= tt < T:
        raise ValueError(f"decode_embed: step {tt} outside [0, {T})")
    return emb.step(ys[:, tt:tt + 1], tt)[:, 0]
