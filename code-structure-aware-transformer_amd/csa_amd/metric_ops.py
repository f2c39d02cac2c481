"""Validation metrics of decoded ids on the device (csrc/csa_metric.hip): the reference's smoothed sentence BLEU-4
(valid_metrices/google_bleu.py compute_bleu(smooth=True) behind bleu_output_transform) and ROUGE-L
(valid_metrices/rouge/rouge.py) restated on token ids, one launch for R hypothesis rows against R / group references.

CUDA int64 rows within csa_seq_metrics_supported (widths 1..256) run the kernel on the current stream with no host
sync; CPU tensors, wider rows and backend="host" run the same definitions as vectorised torch on the tensors' device
(no sync there either). Inference only: no autograd."""
import ctypes
from types import SimpleNamespace

import torch

from ._lib import SEQ_METRICS_FIELDS, CsaError, CsaSeqMetricsArgs, check, lib, on_device

FIELDS = ("m1", "m2", "m3", "m4", "poss1", "poss2", "poss3", "poss4", "len_h", "len_r", "lcs", "valid")
BETA = 1.2
assert len(FIELDS) == SEQ_METRICS_FIELDS


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _lengths(x, eos):
    """Index of the first eos per row, or the width."""
    T = x.shape[1]
    idx = torch.arange(T, device=x.device).expand_as(x)
    return torch.where(x == eos, idx, torch.full_like(idx, T)).amin(1) if T else x.new_zeros(x.shape[0])


def bleu_from_counts(m, poss, len_h, len_r):
    """compute_bleu(smooth=True)'s arithmetic in fp64 on (..., 4) match and possible counts and (...) lengths."""
    prec = (m.double() + 1.0) / (poss.double() + 1.0)
    log_sum = torch.zeros_like(prec[..., 0])
    for n in range(4):
        log_sum = log_sum + 0.25 * torch.log(prec[..., n])
    ratio = len_h.double() / len_r.double()
    bp = torch.where(ratio > 1.0, torch.ones_like(ratio), torch.exp(1.0 - 1.0 / ratio))
    return torch.exp(log_sum) * bp


def seq_metrics_host(hyp, ref, eos_id, group):
    """The fallback: the kernel's definitions as vectorised torch on hyp's device. hyp (R, Th), ref (R / group, Tr).
    O(R T^2) memory per n-gram order (every pair of positions is compared) and Tr steps of (R, Th) ops for the LCS."""
    R, Th = hyp.shape
    dev = hyp.device
    ref = ref.repeat_interleave(group, 0) if group > 1 else ref
    Tr = ref.shape[1]
    lh0, lr = _lengths(hyp, eos_id), _lengths(ref, eos_id)
    valid = lr > 0
    live = valid & (lh0 > 0)  # rows with anything to match
    lh = lh0.clamp(min=1)
    ih = torch.arange(Th, device=dev)
    ir = torch.arange(Tr, device=dev)
    m = torch.zeros(R, 4, dtype=torch.int64, device=dev)
    hh = torch.ones(R, Th, Th, dtype=torch.bool, device=dev)  # [r, i, j]: the n-grams at hyp i and hyp j are equal
    hr = torch.ones(R, Th, Tr, dtype=torch.bool, device=dev)  # [r, i, k]: ... at hyp i and ref k
    before = (ih[None, :] < ih[:, None])[None]  # j < i
    for n in range(1, 5):
        k = n - 1  # extend the (n-1)-gram equality by the tokens at offset k; positions past the width never start one
        eh = torch.zeros_like(hh)
        er = torch.zeros_like(hr)
        if Th > k:
            eh[:, :Th - k, :Th - k] = hyp[:, k:, None] == hyp[:, None, k:]
            if Tr > k:
                er[:, :Th - k, :Tr - k] = hyp[:, k:, None] == ref[:, None, k:]
        hh &= eh
        hr &= er
        start_h = ih[None, :] + n <= lh0[:, None]  # (R, Th): an n-gram starts here
        start_r = ir[None, :] + n <= lr[:, None]
        cb = (hh & before & start_h[:, None, :]).sum(2)
        cr = (hr & start_r[:, None, :]).sum(2)
        m[:, k] = ((cb < cr) & start_h & live[:, None]).sum(1)
    # LCS: one row of the DP per reference token; row[i] = max(cand[0..i]), cand[i] = prev[i-1] + 1 on a match else prev[i]
    prev = torch.zeros(R, Th + 1, dtype=torch.int64, device=dev)
    in_h = ih[None, :] < lh0[:, None]
    for k in range(Tr):
        match = (hyp == ref[:, k, None]) & in_h & (k < lr)[:, None]
        cand = torch.where(match, prev[:, :-1] + 1, prev[:, 1:])
        prev = torch.cat([prev[:, :1], torch.cummax(cand, 1).values], 1) if Th else prev
    lcs = torch.where(live, prev.gather(1, lh0[:, None])[:, 0], torch.zeros_like(lh0))
    poss = (lh[:, None] - torch.arange(4, device=dev)[None, :]).clamp(min=0)
    lr1 = lr.clamp(min=1)
    bleu = bleu_from_counts(m, poss, lh, lr1)
    p, r = lcs.double() / lh.double(), lcs.double() / lr1.double()
    b2 = BETA ** 2
    rouge = torch.where(lcs > 0, ((1 + b2) * p * r) / (r + b2 * p).clamp(min=1e-300), torch.zeros_like(p))
    stats = torch.cat([m, poss, lh[:, None], lr[:, None], lcs[:, None], torch.ones_like(lcs)[:, None]], 1)
    stats = (stats * valid[:, None]).to(torch.int32)
    zero = torch.zeros_like(bleu)
    return SimpleNamespace(stats=stats, bleu=torch.where(valid, bleu, zero), rouge=torch.where(valid, rouge, zero))


def _rows(x, what):
    """(..., T) int64 -> a (rows, T) view with a contiguous last dim and one row stride of at least T (a copy only
    where no such view exists: a strided last dim, or rows that overlap as an expanded row's do)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() not in (2, 3):
        raise ValueError(f"seq_metrics: {what} must be an int64 tensor of 2 or 3 dims")
    x = x.reshape(-1, x.shape[-1])  # a view where the leading dims collapse, as (B, S, T)[:, :, 1:] does
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def seq_metrics(hyp, ref, eos_id=3, group=1, backend=None):
    """Sentence BLEU-4 and ROUGE-L of decoded ids. hyp (R, Th) int64, or (B, S, Th) with group=S; ref (B, Tr) int64 on
    the same device, R = B * group, hypothesis row r scored against reference r // group. Views are taken as they are
    (ys[:, 1:], a sampler's (B, S, T-1)): only the last dim must be contiguous.

    -> namespace(stats (R, 12) int32 with the columns FIELDS, bleu (R,) fp64, rouge (R,) fp64). A row's length is the
    index of its first eos_id (none: the width); an empty hypothesis is the reference's placeholder token (len_h 1, no
    match); a row whose reference is empty has valid = 0 and zeros everywhere.

    backend None: the kernel for CUDA tensors of widths 1..256, otherwise the torch fallback; "host" forces the
    fallback; "device" raises where the kernel cannot run. Neither path synchronises."""
    if backend not in (None, "host", "device"):
        raise ValueError("seq_metrics: backend is None, 'host' or 'device'")
    if isinstance(hyp, torch.Tensor) and hyp.dim() == 3 and hyp.shape[1] != group:
        raise ValueError("seq_metrics: a (B, S, T) hypothesis tensor needs group=S")
    hyp, ref = _rows(hyp, "hyp"), _rows(ref, "ref")
    group, eos_id = int(group), int(eos_id)
    R, Th = hyp.shape
    B, Tr = ref.shape
    if group < 1 or R != B * group:
        raise ValueError(f"seq_metrics: {R} hypothesis rows are not group={group} times {B} reference rows")
    if ref.device != hyp.device:
        raise ValueError("seq_metrics: hyp and ref must be on one device")
    dev = hyp.device
    can = hyp.is_cuda and bool(lib().csa_seq_metrics_supported(Th, Tr))
    if backend == "device" and not can:
        raise CsaError("seq_metrics: the kernel needs CUDA tensors and widths in [1, 256] (csa_seq_metrics_supported)")
    if backend == "host" or not can:
        return seq_metrics_host(hyp, ref, eos_id, group)
    stats = torch.empty(R, SEQ_METRICS_FIELDS, dtype=torch.int32, device=dev)
    bleu = torch.empty(R, dtype=torch.float64, device=dev)
    rouge = torch.empty(R, dtype=torch.float64, device=dev)
    a = CsaSeqMetricsArgs(hyp=hyp.data_ptr(), rows=R, Th=Th, hyp_stride=hyp.stride(0) if R > 1 else max(hyp.stride(0), Th),
                          ref=ref.data_ptr(), Tr=Tr, ref_stride=ref.stride(0) if B > 1 else max(ref.stride(0), Tr),
                          group=group, eos_id=eos_id, stats=stats.data_ptr(), bleu=bleu.data_ptr(),
                          rouge=rouge.data_ptr())
    with on_device(dev):
        check(lib().csa_seq_metrics(ctypes.byref(a), _stream(dev)), "csa_seq_metrics")
    return SimpleNamespace(stats=stats, bleu=bleu, rouge=rouge)
