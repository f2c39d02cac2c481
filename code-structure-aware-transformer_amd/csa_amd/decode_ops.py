"""One KV-cached decode step's non-GEMM ops (csrc/csa_decode.hip, ABI v10): single-query attention against a
K/V cache or a projected memory (csa_decode_attn) and the row argmax of the last-position logits written in
place into the token buffer (csa_argmax_rows). Inference only: no autograd.

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


def _decode_attention_hip(q, K, V, length, key_mask, k_new, v_new, t, scale):
    B, H, hd = q.shape
    out = torch.empty(B, H * hd, device=q.device, dtype=torch.float32)
    a = DecodeAttnArgs(B=B, H=H, hd=hd, len=length, t=t if k_new is not None else 0,
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
        check(lib().csa_decode_attn(ctypes.byref(a), _stream(q.device)), "csa_decode_attn")
    return out


def _decode_attention_ref(q, K, V, length, key_mask, k_new, v_new, t, scale):
    B, H, hd = q.shape
    if k_new is not None:
        K[:, :, t] = k_new
        V[:, :, t] = v_new
    m = None
    if key_mask is not None:
        km = key_mask[..., :length].ne(0).view(B, -1, 1, length)  # (B, 1 | H, 1, length)
        m = torch.zeros(km.shape, dtype=q.dtype, device=q.device).masked_fill_(km, float("-inf"))
    o = F.scaled_dot_product_attention(q.unsqueeze(2), K[:, :, :length], V[:, :, :length], m, scale=scale)
    return o.reshape(B, H * hd)


def decode_attention(q, K, V, length=None, key_mask=None, k_new=None, v_new=None, t=None, scale=None):
    """Single-query attention of one decode step.

    q (B,H,hd); K, V (B,H,>=length,hd) views (any batch / head / key strides, hd contiguous); key_mask optional
    (B,>=length) uint8, or (B,H,>=length) for a per-head mask, last dim contiguous, non-zero = masked key. Returns
    (B, H*hd) contiguous.
    Append mode (k_new, v_new (B,H,hd) and t given): the rows are stored into K[:, :, t] / V[:, :, t] and serve
    as key t; length is t + 1."""
    B, H, hd = q.shape
    if (k_new is None) != (v_new is None) or (k_new is not None and t is None):
        raise ValueError("decode_attention: k_new, v_new and t go together")
    if k_new is not None:
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
    if _hip_ok(q, hd) and all(x.is_cuda and x.dtype == torch.float32 for x in ts):
        return _decode_attention_hip(q, K, V, length, key_mask, k_new, v_new, t, scale)
    return _decode_attention_ref(q, K, V, length, key_mask, k_new, v_new, t, scale)


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


def argmax_rows(x, out=None, is_pad=None, pad_id=0, maxval=None):
    """Row argmax of x (rows, V) into `out` (rows,) int64, which may be a strided column such as ys[:, t+1];
    ties go to the lowest index. Optionally is_pad (rows,) uint8 (strided) receives (index == pad_id) and maxval
    (rows,) fp32 contiguous the row maximum. Returns out."""
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
