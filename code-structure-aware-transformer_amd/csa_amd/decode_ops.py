"""One KV-cached decode step's non-GEMM ops (csrc/csa_decode.hip, ABI v10): single-query attention against a
K/V cache or a projected memory (csa_decode_attn) and the row argmax of the last-position logits written in
place into the token buffer (csa_argmax_rows). Inference only: no autograd.

Device-stepped calls (the captured decode step of CachedGreedyGenerator(graph=True)): where the step index is given as a
1-element int32 tensor instead of an int, the HIP kernels read it on the device (csa_decode_attn_step,
csa_argmax_rows_step, csa_decode_embed) and the host never learns its value, so the same launch serves every step.

fp32 CUDA tensors with a supported head dim run the HIP kernels; CPU tensors, other dtypes or an unsupported
head dim run the same cached algorithm on F.scaled_dot_product_attention / torch.max over the same views.

Beam search (csrc/csa_beam.hip and the BEAM form of the attention kernel): decode_attention takes an ancestry table
(anc=) or a row group sharing one memory (kv_group=), beam_row_topk gives each row's log-sum-exp and top-W logits and
beam_select merges them per AST and rewrites the hypotheses' state in place. Each has the same kind of torch fallback,
so the whole search also runs on the CPU.

Sampled decoding (csrc/csa_sample.hip): sample_rows filters each row of the logits by temperature, top-k and top-p,
draws one token by Gumbel-max from a stateless Philox stream and writes it in place with its log-probability; its
torch fallback restates the same rule, Philox included, in integer tensor ops.

Decoding constraints (csrc/csa_constrain.hip): constrain_rows rewrites the logits in place in front of any of the three
selections (repetition penalty, no-repeat n-gram, minimum length, suppressed ids); its torch fallback is bitwise the
kernel.

Early stop at EOS (csrc/csa_decode.hip): argmax_rows(..., fin=, eos_id=) is the device-stepped argmax with a finished
flag per row (csa_argmax_rows_fin_step) and decode_advance ends a step in place of the counter's increment: it counts
the step and parks the counter at -1 once every row has finished (csa_decode_advance); both fallbacks are bitwise the
kernels."""
import ctypes

import torch
import torch.nn.functional as F

from ._lib import BeamSelectArgs, ConstrainRowsArgs, DecodeAttnArgs, SampleRowsArgs, check, lib, on_device
from .ops import _stream


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _hip_ok(q, hd):
    return q.is_cuda and q.dtype == torch.float32 and bool(lib().csa_decode_attn_supported(hd))


def _is_step(t):
    return isinstance(t, torch.Tensor)


def _rows_hip_ok(x):
    """fp32 CUDA contiguous rows (at least one column): what the row kernels (argmax, top-W) take."""
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] >= 1


def _check_step(t, device, what):
    if t.dtype != torch.int32 or t.numel() != 1 or t.device != device:
        raise ValueError(f"{what}: the device step must be a 1-element int32 tensor on the tensors' device")


def _step_value(t, lo, hi, what):
    """The host-side value of a step given as an int or a counter tensor (fallback paths only: reading the counter
    is not for a captured graph)."""
    tt = int(t.item()) if _is_step(t) else int(t)
    if not lo <= tt < hi:
        raise ValueError(f"{what}: step {tt} outside [{lo}, {hi})")
    return tt


def _decode_attention_hip(q, K, V, length, key_mask, k_new, v_new, t, scale, out=None, anc=None, kv_group=1):
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
        if anc is not None or kv_group != 1:
            check(lib().csa_decode_attn_beam(ctypes.byref(a), _ptr(t) if step else None, _ptr(anc),
                                             anc.stride(0) if anc is not None else 0, kv_group, _stream(q.device)),
                  "csa_decode_attn_beam")
        elif step:  # length is the capacity; the kernel reads t and attends to t + 1 keys
            check(lib().csa_decode_attn_step(ctypes.byref(a), _ptr(t), _stream(q.device)), "csa_decode_attn_step")
        else:
            check(lib().csa_decode_attn(ctypes.byref(a), _stream(q.device)), "csa_decode_attn")
    return out


def _decode_attention_ref(q, K, V, length, key_mask, k_new, v_new, t, scale, out=None, anc=None, kv_group=1):
    B, H, hd = q.shape
    if _is_step(t):  # length is the capacity
        t = _step_value(t, 0, length, "decode_attention")
        length = t + 1
    if k_new is not None:
        K[:, :, t] = k_new
        V[:, :, t] = v_new
    if anc is not None:  # key j < t of row r from cache row anc[r, j], key t from row r itself: a physical gather
        rows = anc[:, :length].long().clone()
        rows[:, t] = torch.arange(B, device=q.device)
        ix = (rows[:, None, :], torch.arange(H, device=q.device)[None, :, None],
              torch.arange(length, device=q.device)[None, None, :])
        K, V = K[ix], V[ix]
    elif kv_group != 1:  # the rows of a group share batch index r // kv_group
        K, V = K.repeat_interleave(kv_group, 0), V.repeat_interleave(kv_group, 0)
        key_mask = None if key_mask is None else key_mask.repeat_interleave(kv_group, 0)
    m = None
    if key_mask is not None:
        km = key_mask[..., :length].ne(0).view(B, -1, 1, length)  # (B, 1 | H, 1, length)
        m = torch.zeros(km.shape, dtype=q.dtype, device=q.device).masked_fill_(km, float("-inf"))
    o = F.scaled_dot_product_attention(q.unsqueeze(2), K[:, :, :length], V[:, :, :length], m, scale=scale)
    o = o.reshape(B, H * hd)
    return o if out is None else out.copy_(o)


def decode_attention(q, K, V, length=None, key_mask=None, k_new=None, v_new=None, t=None, scale=None, out=None,
                     anc=None, kv_group=1):
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
    out: optional (B, H*hd) fp32 contiguous tensor to receive the result.
    Beam search, B = R hypothesis rows:
    anc (R, >= length) int32, append mode only: key / value j < t of row r is read from cache row anc[r, j] instead of
    row r (key t from k_new / v_new, stored at row r as always), the mask byte stays key_mask[r, j]; no cache row moves.
    kv_group = W > 1, without anc: K, V and key_mask hold R / W batch rows and row r reads row r // W, the one memory
    projection of its AST."""
    B, H, hd = q.shape
    kv_group = int(kv_group)
    if kv_group < 1 or (kv_group != 1 and (K.shape[0] * kv_group != B or V.shape[0] * kv_group != B)):
        raise ValueError("decode_attention: kv_group must divide the rows of q, with K and V holding B / kv_group rows")
    if anc is not None and (kv_group != 1 or k_new is None or anc.dtype != torch.int32 or anc.dim() != 2
                            or anc.shape[0] != B or anc.stride(1) != 1 or anc.device != q.device):
        raise ValueError("decode_attention: anc is a (B, >= length) int32 table on q's device with a contiguous last "
                         "dim, for append mode with kv_group == 1")
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
    if not 1 <= length <= K.shape[2] or (key_mask is not None and key_mask.shape[-1] < length) or (
            anc is not None and anc.shape[1] < length):
        raise ValueError("decode_attention: length outside the keys / mask / ancestry table given")
    if key_mask is not None and (key_mask.dtype != torch.uint8 or key_mask.stride(-1) != 1
                                 or key_mask.shape[:-1] not in ((B // kv_group,), (B // kv_group, H))):
        raise ValueError("decode_attention: key_mask must be (B, L) or (B, H, L) uint8 with a contiguous last dim "
                         "(B / kv_group rows with a group)")
    scale = float(hd) ** -0.5 if scale is None else float(scale)
    ts = [x for x in (q, K, V, k_new, v_new) if x is not None]
    if any(x.stride(-1) != 1 for x in ts):
        raise ValueError("decode_attention: the head dim must be contiguous")
    if out is not None and (out.shape != (B, H * hd) or out.dtype != q.dtype or out.device != q.device
                            or not out.is_contiguous()):
        raise ValueError("decode_attention: out must be (B, H*hd) contiguous, of q's dtype and device")
    extra = () if out is None else (out,)
    if anc is not None or kv_group != 1:
        extra = (out, anc, kv_group)
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


def _argmax_rows_step(x, ys, pad, pad_id, t_dev, head_pad, fin=None, eos_id=None):
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
    if fin is not None and (fin.dtype != torch.uint8 or fin.shape != (rows,) or not fin.is_contiguous()
                            or fin.device != x.device):
        raise ValueError("argmax_rows: fin is a (rows,) uint8 contiguous tensor on x's device")
    _check_step(t_dev, x.device, "argmax_rows")
    eos = -1 if eos_id is None else int(eos_id)
    if _rows_hip_ok(x):
        tail = (_ptr(pad), pad.stride(0) if pad is not None else 0, _ptr(head_pad),
                head_pad.shape[1] if head_pad is not None else 0, pad_id)
        with on_device(x.device):
            if fin is None:
                check(lib().csa_argmax_rows_step(_ptr(x), rows, V, _ptr(ys), ys.stride(0), T, *tail, _ptr(t_dev),
                                                 _stream(x.device)), "csa_argmax_rows_step")
            else:
                check(lib().csa_argmax_rows_fin_step(_ptr(x), rows, V, _ptr(ys), ys.stride(0), T, *tail, _ptr(fin), eos,
                                                     _ptr(t_dev), _stream(x.device)), "csa_argmax_rows_fin_step")
        return ys
    col = _step_value(t_dev, 0, T - 1, "argmax_rows") + 1  # column in [1, T)
    _argmax_rows_ref(x, ys[:, col], None if pad is None else pad[:, col], pad_id, None)
    if fin is not None:  # a finished row takes PAD; a live row that drew eos_id is finished from the next step on
        done = fin != 0
        ys[:, col].masked_fill_(done, pad_id)
        if pad is not None:
            pad[:, col] = ys[:, col] == pad_id
        fin.masked_fill_(~done & (ys[:, col] == eos), 1)
    if head_pad is not None:
        _head_view(head_pad, rows)[:, :, col] = ys[:, col] == pad_id
    return ys


def decode_advance(fin, t_dev, state, T):
    """The end of an early-stopping decode step, in place of the counter's increment (csa_decode_advance,
    include/csa_hip.h). fin (R,) uint8, any non-zero byte = finished, a contiguous view of any alignment; t_dev the
    1-element int32 step counter; state (4,) int32 = {all_prev, steps_run, parked, reserved}, zeroed before step 0; T the
    token buffer's columns. Parked: nothing changes. Otherwise steps_run += 1 and the counter parks at -1 (parked = 1)
    when all_prev is set or step t was the last (t + 1 >= T - 1), else moves to t + 1 with all_prev = every row finished.
    The step kernels store nothing for a negative counter, so a parked step is harmless. CUDA tensors run the kernel;
    CPU tensors run the same rule on the host."""
    dev = t_dev.device
    _check_step(t_dev, dev, "decode_advance")
    if (fin.dtype != torch.uint8 or fin.dim() != 1 or (fin.numel() > 1 and fin.stride(0) != 1) or fin.device != dev
            or state.dtype != torch.int32 or state.shape != (4,) or not state.is_contiguous() or state.device != dev):
        raise ValueError("decode_advance: fin (R,) uint8 with unit stride and state (4,) int32 contiguous, both on the "
                         "counter's device")
    T = int(T)
    if T < 2:
        raise ValueError("decode_advance: T >= 2")
    if dev.type == "cuda":
        with on_device(dev):
            check(lib().csa_decode_advance(_ptr(fin), fin.numel(), T, _ptr(t_dev), _ptr(state), _stream(dev)),
                  "csa_decode_advance")
        return
    all_prev, steps, parked, _ = state.tolist()
    if parked:
        return
    t = int(t_dev.item())
    state[1] = steps + 1
    if all_prev or t + 1 >= T - 1:
        t_dev.fill_(-1)
        state[2] = 1
    else:
        t_dev.fill_(t + 1)
        state[0] = int(bool((fin != 0).all()))


def argmax_rows(x, out=None, is_pad=None, pad_id=0, maxval=None, t_dev=None, head_pad=None, fin=None, eos_id=None):
    """Row argmax of x (rows, V) into `out` (rows,) int64, which may be a strided column such as ys[:, t+1];
    ties go to the lowest index. Optionally is_pad (rows,) uint8 (strided) receives (index == pad_id) and maxval
    (rows,) fp32 contiguous the row maximum. Returns out.
    Device-stepped (t_dev a 1-element int32 tensor): out is the whole (rows, T) token buffer and is_pad the whole
    (rows, T) mask; the kernel reads t and writes column t + 1 of both and, when head_pad (rows, H, T) is given, the
    same byte into head_pad.view(H, rows, T)[:, r, t + 1], the column BaseDecoder.step would copy from is_pad at the
    top of step t + 1. A column outside [1, T) stores nothing.
    fin (rows,) uint8 with eos_id, device-stepped only (csa_argmax_rows_fin_step): a row with fin != 0 takes pad_id and
    PAD byte 1 in is_pad and head_pad whatever its logits; a live row whose argmax is eos_id (None: never) gets
    fin = 1, so it is finished from the next step on."""
    if t_dev is not None:
        if out is None or maxval is not None:
            raise ValueError("argmax_rows: with t_dev, out is required and maxval is not available")
        return _argmax_rows_step(x, out, is_pad, pad_id, t_dev, head_pad, fin, eos_id)
    if head_pad is not None or fin is not None:
        raise ValueError("argmax_rows: head_pad and fin go with t_dev")
    rows, _ = x.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=x.device)
    if out.dtype != torch.int64 or out.shape != (rows,) or (is_pad is not None and (
            is_pad.dtype != torch.uint8 or is_pad.shape != (rows,))) or (maxval is not None and (
            maxval.dtype != torch.float32 or maxval.shape != (rows,) or not maxval.is_contiguous())):
        raise ValueError("argmax_rows: out (rows,) int64, is_pad (rows,) uint8, maxval (rows,) fp32 contiguous")
    if _rows_hip_ok(x):
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
    tt = _step_value(t, 0, T, "decode_embed")
    return emb.step(ys[:, tt:tt + 1], tt)[:, 0]


# ---- beam search: per-row top-W and log-sum-exp, per-AST merge with the in-place state update ----

def _beam_row_topk_ref(z, W, lse, topv, topi):
    zf = z.float()
    lse.copy_(torch.logsumexp(zf, dim=1))
    v, i = torch.sort(zf, dim=1, descending=True, stable=True)  # equal values keep their index order
    topv.copy_(v[:, :W])
    topi.copy_(i[:, :W])


def beam_row_topk(z, W, lse=None, topv=None, topi=None, t_dev=None, t_end=None):
    """Per row of the logits z (rows, V), V >= W: lse (rows,) fp32 = log sum exp, topv (rows, W) fp32 the W largest
    logits in descending order and topi (rows, W) int32 their indices, the lowest index first among equal values (an
    all -inf row gives 0 .. W-1). Returns (lse, topv, topi); the three are allocated unless given (contiguous).
    t_dev (1-element int32 counter) with t_end: the HIP kernel stores nothing unless 0 <= t < t_end; off the HIP path
    the host reads the counter and a step outside that range raises."""
    rows, V = z.shape
    W = int(W)
    if not 1 <= W <= 8:
        raise ValueError("beam_row_topk: the beam width must be in [1, 8]")
    if V < W:
        raise ValueError("beam_row_topk: V must be at least W")
    if (t_dev is None) != (t_end is None):
        raise ValueError("beam_row_topk: t_dev and t_end go together")
    if t_dev is not None:
        _check_step(t_dev, z.device, "beam_row_topk")
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=z.device)
    lse = new((rows,), torch.float32) if lse is None else lse
    topv = new((rows, W), torch.float32) if topv is None else topv
    topi = new((rows, W), torch.int32) if topi is None else topi
    for x, shape, dt in ((lse, (rows,), torch.float32), (topv, (rows, W), torch.float32), (topi, (rows, W), torch.int32)):
        if x.shape != shape or x.dtype != dt or x.device != z.device or not x.is_contiguous():
            raise ValueError("beam_row_topk: lse (rows,) fp32, topv (rows, W) fp32, topi (rows, W) int32, contiguous, "
                             "on z's device")
    if _rows_hip_ok(z):
        with on_device(z.device):
            check(lib().csa_beam_row_topk(_ptr(z), rows, V, W, _ptr(lse), _ptr(topv), _ptr(topi), _ptr(t_dev),
                                          0 if t_end is None else int(t_end), _stream(z.device)), "csa_beam_row_topk")
    else:
        if t_dev is not None:
            _step_value(t_dev, 0, int(t_end), "beam_row_topk")
        _beam_row_topk_ref(z, W, lse, topv, topi)
    return lse, topv, topi


def _beam_select_ref(topv, topi, lse, cum, fin, tokens, pad, anc, t, eos_id, pad_id, parent):
    R, W = topv.shape
    B, dev = R // W, topv.device
    live = fin.view(B, W, 1) == 0
    score = cum.view(B, W, 1) + (topv.view(B, W, W) - lse.view(B, W, 1))
    score = torch.where(live, score, cum.view(B, W, 1).expand(B, W, W))
    score = torch.where(score > float("-inf"), score, torch.full_like(score, float("-inf")))  # NaN too
    tok = torch.where(live, topi.view(B, W, W).long(), torch.full((B, W, W), pad_id, dtype=torch.long, device=dev))
    offered = live | (torch.arange(W, device=dev).view(1, 1, W) == 0)
    row = torch.arange(W, device=dev).view(1, W, 1).expand(B, W, W)
    score, tok, offered, row = (x.reshape(B, W * W) for x in (score, tok, offered, row))
    # score descending, then parent row, then token, the offered candidates first: stable sorts, last key first
    order = torch.argsort(tok, dim=1, stable=True)
    for key, desc in ((row, False), (score, True), (offered.to(torch.int8), True)):
        order = order.gather(1, torch.argsort(key.gather(1, order), dim=1, descending=desc, stable=True))
    best = order[:, :W]
    p_local = row.gather(1, best)
    prow = (p_local + W * torch.arange(B, device=dev).view(B, 1)).reshape(R)
    new_tok = tok.gather(1, best).reshape(R)
    new_fin = (fin[prow] != 0) | (new_tok == eos_id)
    new_cum = score.gather(1, best).reshape(R)
    tokens[:, :t + 1] = tokens[prow, :t + 1]
    pad[:, :t + 1] = pad[prow, :t + 1]
    anc[:, :t] = anc[prow, :t]
    tokens[:, t + 1] = new_tok
    pad[:, t + 1] = new_tok == pad_id
    anc[:, t] = prow
    cum.copy_(new_cum)
    fin.copy_(new_fin)
    if parent is not None:
        parent.copy_(prow)


def beam_select(topv, topi, lse, cum, fin, tokens, pad, anc, t, eos_id=None, pad_id=0, parent=None):
    """One beam step of every AST, in place (rows r = b * W + w; W = topv.shape[1]).

    topv / topi (R, W) and lse (R,) from beam_row_topk; cum (R,) fp32 and fin (R,) uint8 the hypotheses' cumulative
    log-probability and finished flag; tokens (R, T) int64, pad (R, T) uint8 and anc (R, T) int32 (row strides free,
    last dim contiguous) the token buffer, the PAD key mask and the ancestry table. A live row offers
    (cum + (topv - lse), topi) W times, a finished row only (cum, pad_id); the best W per AST (score descending, then
    parent row, then token) become its rows: a child takes its parent's columns 0..t of tokens and pad and 0..t-1 of
    anc, then tokens[:, t+1], pad[:, t+1] = (token == pad_id), anc[:, t] = the parent row, cum and
    fin = parent finished or token == eos_id (None: never). parent (R,) int32, optional, receives the parent rows.
    t: the 1-element int32 counter (the HIP kernel reads it; a step outside [0, T-1) stores nothing) or an int."""
    R, W = topv.shape
    T = tokens.shape[1] if tokens.dim() == 2 else -1
    dev = topv.device
    eos = -1 if eos_id is None else int(eos_id)

    def bad(x, shape, dt, contiguous=True):
        return (x.shape != shape or x.dtype != dt or x.device != dev
                or (not x.is_contiguous() if contiguous else x.stride(-1) != 1))
    if not 1 <= W <= 8 or R % W != 0:
        raise ValueError("beam_select: the beam width topv.shape[1] must be in [1, 8] and divide the rows")
    if (bad(topv, (R, W), torch.float32) or bad(topi, (R, W), torch.int32) or bad(lse, (R,), torch.float32)
            or bad(cum, (R,), torch.float32) or bad(fin, (R,), torch.uint8) or bad(tokens, (R, T), torch.int64, False)
            or bad(pad, (R, T), torch.uint8, False) or bad(anc, (R, T), torch.int32, False)
            or (parent is not None and bad(parent, (R,), torch.int32))):
        raise ValueError("beam_select: topv (R, W) fp32, topi (R, W) int32, lse / cum (R,) fp32, fin (R,) uint8, tokens "
                         "(R, T) int64, pad (R, T) uint8, anc (R, T) int32, parent (R,) int32, all on one device")
    if _is_step(t):
        _check_step(t, dev, "beam_select")
    if topv.is_cuda and bool(lib().csa_beam_supported(W, T)):
        t_dev = t if _is_step(t) else torch.tensor([int(t)], dtype=torch.int32, device=dev)
        a = BeamSelectArgs(B=R // W, W=W, T=T, topv=_ptr(topv), topi=_ptr(topi), lse=_ptr(lse), cum=_ptr(cum),
                           fin=_ptr(fin), tokens=_ptr(tokens), tok_stride=tokens.stride(0), pad=_ptr(pad),
                           pad_stride=pad.stride(0), anc=_ptr(anc), anc_stride=anc.stride(0), parent=_ptr(parent),
                           eos_id=eos, pad_id=int(pad_id), t_dev=_ptr(t_dev))
        with on_device(dev):
            check(lib().csa_beam_select(ctypes.byref(a), _stream(dev)), "csa_beam_select")
    else:
        _beam_select_ref(topv, topi, lse, cum, fin, tokens, pad, anc, _step_value(t, 0, T - 1, "beam_select"), eos,
                         int(pad_id), parent)


# ---- sampled decoding: temperature, top-k, top-p and one Gumbel-max draw per row ----

RNG_SAMPLE = 7  # Philox stream id of the sampling draws (counter word 3 high bits)
_M32 = 0xFFFFFFFF


def _mulhilo(a, x):
    """(hi, lo) 32-bit words of the constant a times the 32-bit values held in the int64 tensor x, without leaving
    int64: a * x is formed from the 16-bit halves of x."""
    pl, ph = a * (x & 0xFFFF), a * (x >> 16)
    low = pl + ((ph & 0xFFFF) << 16)
    return (ph >> 16) + (low >> 32), low & _M32


def _philox4x32(c0, c1, c2, c3, k0, k1, rounds=7):
    """Philox4x32-7 (csrc/csa_common.hpp philox4x32) over int64 tensors holding 32-bit counter words."""
    for _ in range(rounds):
        h0, l0 = _mulhilo(0xD2511F53, c0)
        h1, l1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def _sample_gumbel(rows, V, t, seed, offset, device):
    """g (rows, V) fp32: -log(-log u), u = ((w >> 9) + 0.5) 2^-23, w = word j & 3 of philox({j >> 2, r, t,
    (RNG_SAMPLE << 28) ^ lo32(offset)}, seed)."""
    j = torch.arange(V, dtype=torch.int64, device=device).view(1, V)
    r = torch.arange(rows, dtype=torch.int64, device=device).view(rows, 1)
    zero = torch.zeros(rows, V, dtype=torch.int64, device=device)
    c3 = ((RNG_SAMPLE << 28) ^ (offset & _M32)) & _M32
    words = _philox4x32((j >> 2) + zero, r + zero, zero + (t & _M32), zero + c3, seed & _M32, (seed >> 32) & _M32)
    w = torch.stack(words, 0).gather(0, ((j & 3) + zero).unsqueeze(0))[0]
    u = ((w >> 9).to(torch.float32) + 0.5) * (1.0 / 8388608.0)
    return -torch.log(-torch.log(u))


def _sample_rows_ref(z, ys, pad, fin, t, seed, offset, inv, top_k, top_p, eos, pad_id, logp):
    """csa_sample_rows in plain torch: the same sets and the same fp32 noisy scores; the softmax masses of the top-p
    rule and the log-sum-exp are summed in fp64."""
    rows, V = z.shape
    ninf = float("-inf")
    y = z.float() * torch.tensor(inv, dtype=torch.float32, device=z.device)
    keep = y > ninf  # neither -inf nor NaN
    yc = torch.where(keep, y, torch.full_like(y, ninf))
    ncand = keep.sum(1)
    if top_k > 0:
        srt = torch.sort(yc, dim=1, descending=True)[0]
        theta = srt[:, min(top_k, V) - 1]
        on = (ncand > top_k).unsqueeze(1)
        keep = keep & (~on | (yc >= theta.unsqueeze(1)))
    if top_p < 1.0:
        y2 = torch.where(keep, yc, torch.full_like(yc, ninf)).double()
        srt, order = torch.sort(y2, dim=1, descending=True)
        p = torch.softmax(srt, dim=1)
        p = torch.where(torch.isnan(p), torch.zeros_like(p), p)  # a row without candidates
        before = torch.cumsum(p, 1) - p
        start = torch.ones_like(srt, dtype=torch.bool)
        start[:, 1:] = srt[:, 1:] != srt[:, :-1]
        G = torch.cummax(torch.where(start, before, torch.full_like(before, -1.0)), dim=1)[0]  # the class's first entry
        keep_sorted = G < float(torch.tensor(top_p, dtype=torch.float32))
        keep = keep & torch.zeros_like(keep).scatter(1, order, keep_sorted)
    score = torch.where(keep, y + _sample_gumbel(rows, V, t, seed, offset, z.device), torch.full_like(y, ninf))
    tok = torch.argmax(score, dim=1)  # the first maximal entry
    has = keep.any(1)
    tok = torch.where(has, tok, torch.zeros_like(tok))
    lse = torch.logsumexp(torch.where(keep, y, torch.full_like(y, ninf)).double(), dim=1)
    lp = (y.gather(1, tok.unsqueeze(1))[:, 0].double() - lse).float()
    lp = torch.where(has, lp, torch.full_like(lp, ninf))
    done = fin != 0
    tok = torch.where(done, torch.full_like(tok, pad_id), tok)
    ys[:, t + 1] = tok
    pad[:, t + 1] = tok == pad_id
    if logp is not None:
        logp[:, t] = torch.where(done, torch.zeros_like(lp), lp)
    fin.copy_((done | (tok == eos)).to(torch.uint8))


def sample_rows(z, ys, pad, fin, t_dev, rng, temperature=1.0, top_k=0, top_p=1.0, eos_id=None, pad_id=0, logp=None):
    """One sampled token per row of the last-position logits z (rows, V), in place (csa_sample_rows, include/csa_hip.h).

    y = fl32(z / temperature as a product with fl32(1) / fl32(temperature)); top_k > 0 keeps the entries at or above
    the top_k-th largest value (all ties; off when it covers every candidate), top_p < 1 keeps, of the softmax over
    that set, the classes of equal values whose strictly larger entries hold a mass below top_p; one Gumbel-max draw
    over what is left (Philox stream 7, counter {j >> 2, row, t, offset}, key seed; lowest index on a tie). ys (rows, T)
    int64, pad (rows, T) uint8 (row strides free, last dim contiguous), fin (rows,) uint8: ys[:, t+1] = token,
    pad[:, t+1] = (token == pad_id), fin |= (token == eos_id) (None: never); a finished row takes pad_id. logp
    (rows, T-1) fp32, optional, receives logp[:, t] = the token's log-probability under the filtered distribution
    (0 for a finished row, -inf with token 0 for a row without a candidate). t_dev: the 1-element int32 step counter;
    rng: a 2-element int64 tensor {seed, offset} on z's device, read on the device by the HIP kernel (a captured
    graph draws anew once it is refilled). fp32 CUDA rows within csa_sample_rows_supported run the kernel, which
    stores nothing for a step outside [0, T-1); anything else reads the counter and rng on the host."""
    rows, V = z.shape
    T = ys.shape[1] if ys.dim() == 2 else -1
    dev = z.device
    if (ys.dtype != torch.int64 or ys.dim() != 2 or ys.shape[0] != rows or ys.stride(1) != 1 or ys.device != dev
            or pad.dtype != torch.uint8 or pad.shape != (rows, T) or pad.stride(1) != 1 or pad.device != dev
            or fin.dtype != torch.uint8 or fin.shape != (rows,) or not fin.is_contiguous() or fin.device != dev
            or (logp is not None and (logp.dtype != torch.float32 or logp.shape != (rows, T - 1) or logp.stride(1) != 1
                                      or logp.device != dev))):
        raise ValueError("sample_rows: ys (rows, T) int64, pad (rows, T) uint8, logp (rows, T-1) fp32, each with a "
                         "contiguous last dim, and fin (rows,) uint8 contiguous, all on z's device")
    if rng.dtype != torch.int64 or rng.shape != (2,) or not rng.is_contiguous() or rng.device != dev:
        raise ValueError("sample_rows: rng is a 2-element int64 tensor {seed, offset} on z's device")
    _check_step(t_dev, dev, "sample_rows")
    temperature, top_k, top_p = float(temperature), int(top_k), float(top_p)
    if not temperature > 0.0 or top_k < 0 or not top_p > 0.0 or T < 2:
        raise ValueError("sample_rows: temperature > 0, top_k >= 0 (0: off), top_p > 0 (>= 1: off) and T >= 2")
    inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32))
    eos = -1 if eos_id is None else int(eos_id)
    if _rows_hip_ok(z) and bool(lib().csa_sample_rows_supported(V)):
        a = SampleRowsArgs(logits=_ptr(z), rows=rows, V=V, logits_stride=z.stride(0), ys=_ptr(ys), ys_stride=ys.stride(0),
                           pad=_ptr(pad), pad_stride=pad.stride(0), logp=_ptr(logp),
                           logp_stride=logp.stride(0) if logp is not None else 0, T=T, fin=_ptr(fin),
                           inv_temperature=inv, top_p=min(top_p, 1.0), top_k=min(top_k, 0x7fffffff), eos_id=eos,
                           pad_id=int(pad_id), rng_dev=_ptr(rng), t_dev=_ptr(t_dev))
        with on_device(dev):
            check(lib().csa_sample_rows(ctypes.byref(a), _stream(dev)), "csa_sample_rows")
        return ys
    t = _step_value(t_dev, 0, T - 1, "sample_rows")
    seed, offset = (int(v) & 0xFFFFFFFFFFFFFFFF for v in rng.tolist())
    _sample_rows_ref(z, ys, pad, fin, t, seed, offset, inv, top_k, top_p, eos, int(pad_id), logp)
    return ys


# ---- decoding constraints: repetition penalty, no-repeat n-gram, minimum length and suppressed ids ----

MAX_SUPPRESS = 256  # entries of the suppress list (csa_constrain_rows)


def _constrain_rows_ref(z, ys, t, fin, theta, ngram, min_length, eos, suppress):
    """csa_constrain_rows in plain torch, in place: the same sets, and the penalty as the same two fp32 operations (a
    division and a product by the fp32 theta held in a tensor, so neither becomes a product by a reciprocal), which
    makes it bitwise the kernel."""
    rows, V = z.shape
    dev = z.device
    L = t + 1
    live = torch.ones(rows, 1, dtype=torch.bool, device=dev) if fin is None else (fin == 0).view(rows, 1)
    h = ys[:, :L]
    inr = (h >= 0) & (h < V)

    def marks(tok, on):  # (rows, V) bool: the in-range tokens of tok where on; the others go to a spare column
        m = torch.zeros(rows, V + 1, dtype=torch.bool, device=dev)
        m.scatter_(1, torch.where(on & (tok >= 0) & (tok < V), tok, torch.full_like(tok, V)), True)
        return m[:, :V]

    if theta != 1.0:
        th = torch.tensor(theta, dtype=torch.float32, device=dev)
        zf = z.float()
        z.copy_(torch.where(marks(h, inr) & live, torch.where(zf > 0, zf / th, zf * th).to(z.dtype), z))
    ban = torch.zeros(rows, V, dtype=torch.bool, device=dev)
    if 1 <= ngram <= L:
        match = torch.ones(rows, L - ngram + 1, dtype=torch.bool, device=dev)
        for k in range(ngram - 1):  # h[i + k] == h[L - (n - 1) + k] for every start i at once
            match &= h[:, k:k + L - ngram + 1] == h[:, L - ngram + 1 + k].unsqueeze(1)
        ban |= marks(h[:, ngram - 1:], match)
    if 0 <= eos < V and t < min_length:
        ban[:, eos] = True
    if suppress is not None and suppress.numel():
        s = suppress.long().view(1, -1).expand(rows, -1)
        ban |= marks(s, torch.ones_like(s, dtype=torch.bool))
    z.masked_fill_(ban & live, float("-inf"))


def constrain_rows(z, ys, t, *, fin=None, repetition_penalty=1.0, no_repeat_ngram=0, min_length=0, eos_id=None,
                   suppress=None):
    """Decoding constraints on the last-position logits z (rows, V), in place (csa_constrain_rows, include/csa_hip.h),
    in front of argmax_rows / beam_row_topk / sample_rows, which see a banned token as a -inf logit.

    ys (rows, T) int64 token buffer (row stride free, last dim contiguous); the history of row r at step t is
    ys[r, 0..t], the literal columns. t: the 1-element int32 step counter or an int in [0, T-1). fin (rows,) uint8,
    optional: a row with fin != 0 is left untouched. repetition_penalty theta > 0 (1: off): each distinct in-range
    history token's logit becomes z / theta if z > 0 else z * theta, once. no_repeat_ngram n >= 0 (0: off): a token that
    would complete an n-gram already in the history is banned. min_length: eos_id (None: off) is banned while
    t < min_length. suppress: an int32 tensor of at most 256 ids on z's device, banned at every step (ids outside
    [0, V) are ignored). A ban stores -inf and wins over the penalty. z: rows with a contiguous last dim and a row
    stride >= V. fp32 CUDA rows with T within csa_constrain_rows_supported run the kernel, which stores nothing for a
    counter outside [0, T-1); anything else reads the counter on the host and runs the same fp32 operations in torch,
    bitwise the kernel. Returns z."""
    if (z.dim() != 2 or not z.is_floating_point() or (z.shape[1] > 1 and z.stride(1) != 1)
            or (z.shape[0] > 1 and z.stride(0) < z.shape[1])):
        raise ValueError("constrain_rows: z must be (rows, V) floating point with a contiguous last dim and a row stride "
                         "of at least V")
    rows, V = z.shape
    T = ys.shape[1] if ys.dim() == 2 else -1
    dev = z.device
    if (ys.dtype != torch.int64 or ys.dim() != 2 or ys.shape[0] != rows or ys.stride(1) != 1 or ys.device != dev
            or (fin is not None and (fin.dtype != torch.uint8 or fin.shape != (rows,) or not fin.is_contiguous()
                                     or fin.device != dev))):
        raise ValueError("constrain_rows: ys (rows, T) int64 with a contiguous last dim and fin (rows,) uint8 contiguous, "
                         "on z's device")
    if suppress is not None and (not isinstance(suppress, torch.Tensor) or suppress.dtype != torch.int32
                                 or suppress.dim() != 1 or suppress.numel() > MAX_SUPPRESS
                                 or not suppress.is_contiguous() or suppress.device != dev):
        raise ValueError("constrain_rows: suppress is a contiguous int32 tensor of at most 256 ids on z's device")
    theta = float(torch.tensor(float(repetition_penalty), dtype=torch.float32))  # the fp32 value the kernel takes
    if int(no_repeat_ngram) != no_repeat_ngram or int(min_length) != min_length:
        raise ValueError("constrain_rows: no_repeat_ngram and min_length are integers")
    ngram, min_length = int(no_repeat_ngram), int(min_length)
    if not 0.0 < theta < float("inf") or ngram < 0 or min_length < 0 or T < 2:
        raise ValueError("constrain_rows: repetition_penalty in (0, inf) (1: off), no_repeat_ngram >= 0 (0: off), "
                         "min_length >= 0 and T >= 2")
    eos = -1 if eos_id is None or int(eos_id) < 0 else int(eos_id)
    step = _is_step(t)
    if step:
        _check_step(t, dev, "constrain_rows")
    else:
        t = _step_value(t, 0, T - 1, "constrain_rows")
    if z.is_cuda and z.dtype == torch.float32 and bool(lib().csa_constrain_rows_supported(T)):
        a = ConstrainRowsArgs(logits=_ptr(z), rows=rows, V=V, logits_stride=z.stride(0) if rows > 1 else max(z.stride(0), V),
                              ys=_ptr(ys), ys_stride=ys.stride(0) if rows > 1 else max(ys.stride(0), T), T=T,
                              fin=_ptr(fin), repetition_penalty=theta, no_repeat_ngram=ngram, min_length=min_length,
                              eos_id=eos, suppress=_ptr(suppress) if suppress is not None and suppress.numel() else None,
                              n_suppress=suppress.numel() if suppress is not None else 0,
                              t=0 if step else t, t_dev=_ptr(t) if step else None)
        with on_device(dev):
            check(lib().csa_constrain_rows(ctypes.byref(a), _stream(dev)), "csa_constrain_rows")
        return z
    _constrain_rows_ref(z, ys, _step_value(t, 0, T - 1, "constrain_rows"), fin, theta, ngram, min_length, eos, suppress)
    return z
