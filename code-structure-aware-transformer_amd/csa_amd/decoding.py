"""The decoding strategies over the KV-cached decode step of csa_amd.model (BaseDecoder.step, DecodeCache): cached
greedy, beam search and sampling, their shared constraints and the device-stepped, graph-captured step skeleton.
Only GreedyGenerator has a counterpart in the reference and it stays in csa_amd.model, which re-exports the names of
this module."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from .data import BOS, EOS
from .model import PAD, GreedyGenerator


@dataclass(frozen=True)
class DecodingConstraints:
    """Which tokens a decoding step may choose, for CachedGreedyGenerator, BeamSearchGenerator and SamplingGenerator
    (decode_ops.constrain_rows, csrc/csa_constrain.hip): a frozen, hashable value.

    repetition_penalty theta > 0 (1: off): the logit z of every token already in the row's history, BOS included,
    becomes z / theta if z > 0 else z * theta, once however often the token occurs. no_repeat_ngram_size n >= 0 (0: off):
    a token that would complete an n-gram the history already holds is banned. min_length: eos_id is banned at the
    steps t < min_length, so an output holds at least min_length tokens before its EOS (off at 0 or with eos_id None).
    suppress_ids: at most 256 ids banned at every step. A banned token is a -inf logit to the selection that follows,
    which renormalises over what is left. `active` is False when every rule is off; the generators then run exactly
    the launches they run without constraints."""

    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_length: int = 0
    suppress_ids: tuple = ()
    eos_id: Optional[int] = EOS

    MAX_SUPPRESS = 256

    def __post_init__(self):
        theta = float(self.repetition_penalty)
        if not 0.0 < theta < float("inf"):
            raise ValueError("DecodingConstraints: repetition_penalty must be positive and finite (1 turns it off)")
        for name in ("no_repeat_ngram_size", "min_length"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < 0:
                raise ValueError(f"DecodingConstraints: {name} must be a non-negative integer (0 turns it off)")
        ids, eos = tuple(self.suppress_ids), self.eos_id
        if len(ids) > self.MAX_SUPPRESS or any(isinstance(i, bool) or int(i) != i or not 0 <= i < 2 ** 31 for i in ids):
            raise ValueError("DecodingConstraints: suppress_ids holds at most 256 non-negative integer ids")
        if eos is not None and (isinstance(eos, bool) or int(eos) != eos or eos < 0):
            raise ValueError("DecodingConstraints: eos_id must be a non-negative integer or None")
        for name, v in (("repetition_penalty", theta), ("no_repeat_ngram_size", int(self.no_repeat_ngram_size)),
                        ("min_length", int(self.min_length)), ("suppress_ids", tuple(int(i) for i in ids)),
                        ("eos_id", None if eos is None else int(eos))):
            object.__setattr__(self, name, v)  # the normalised value (frozen: no plain assignment)

    @property
    def active(self):
        return (self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or bool(self.suppress_ids)
                or (self.min_length > 0 and self.eos_id is not None))

    def apply(self, logits, ys, t, fin=None, suppress=None):
        """One constrain_rows call with this value's rules; suppress: suppress_tensor(device) made once."""
        from .decode_ops import constrain_rows
        return constrain_rows(logits, ys, t, fin=fin, repetition_penalty=self.repetition_penalty,
                              no_repeat_ngram=self.no_repeat_ngram_size, min_length=self.min_length, eos_id=self.eos_id,
                              suppress=suppress)

    def suppress_tensor(self, device):
        """The suppress list as the static int32 device tensor that the kernel reads, or None for an empty list."""
        return torch.tensor(self.suppress_ids, dtype=torch.int32, device=device) if self.suppress_ids else None


class _SteppedDecoding:
    """What CachedGreedyGenerator, BeamSearchGenerator and SamplingGenerator share: the device-stepped decode step and
    the state it runs on. Every kernel of _device_step reads the step from the 4-byte device counter e.t_dev, so every
    step issues the same launches: embedding, BaseDecoder.step, the generator's linear, the constraints if any, the
    generator's own _select(e, logits), and the counter's advance. A generator supplies _select and, where it has
    something of its own, _own_state(e, z, return_logp), _own_reset(e), _key_extras() and _check_capture(enc).

    graph=True (CUDA memory): the step is captured once per (device, B, S, max_tgt_len, the generator's key extras,
    return_logp, constraints, eos_id, early_stop, parameter addresses) as one single-stream torch.cuda.CUDAGraph over
    static buffers and replayed max_tgt_len - 1 times per call. `captures` counts the graphs captured. Otherwise the
    same step runs eagerly on a fresh state (_prepare decides and returns the reset state either way).

    constraints= (a DecodingConstraints): when active, one decode_ops.constrain_rows call sits between generator.linear
    and the selection of every step, the value joins the graph key and the suppress list is a static device tensor of
    the state; None or an inactive value changes nothing.

    early_stop=True (needs an eos_id, so a finished flag e.fin per row) is one rule for the three generators: decoding
    stops after the first step that BEGAN with every row finished, one step after the step s that finished the last
    row, so steps 0..s+1 run; without such a step all max_tgt_len - 1 run. The extra step is the one after which the
    state is a fixed point (for the beam, the step in which the selection orders the all-finished hypotheses by cum), so
    ids, scores and log-probabilities are bitwise those of the full run; columns never written stay PAD / 0 as _reset
    leaves them. On the device the rule is a latch: the step ends with decode_ops.decode_advance in place of the
    counter's increment, which counts the step in the state words e.stop = {all_prev, steps_run, parked, 0} and parks
    the counter at -1; every step kernel returns on a negative counter, so a surplus replay stores nothing. The host
    (_run_steps) issues replays in chunks of poll_every, copies the state words to a pinned buffer after each chunk
    (outside the graph, same stream, non-blocking) and, before issuing chunk k + 2, waits for chunk k's copy and stops
    if it reports parked: at most two chunks are ever in flight and no kernel waits on the host. last_steps_run is the
    latch's count after the call (max_tgt_len - 1 without early_stop), exact whatever the chunking; last_replays is
    the number of steps issued, at most last_steps_run + 2 * poll_every. False keeps the launches, the graph key and
    the captured graph of a generator built without the keyword."""

    MAX_GRAPHS = 4  # captured (shape, weights) entries kept per generator; the oldest is evicted
    POLL_EVERY = 2  # replays per chunk of an early-stopping graph=True call: the fastest of 2, 4 and 8
                    # (tools/bench_early_stop.py, profiles/early_stop_decode.json)
    FIN_WITHOUT_EOS = True  # the state holds a finished flag per row even with eos_id None (it then stays 0)

    def _init_stepped(self, model, max_tgt_len, multi_gpu, eos_id, graph, early_stop, constraints, **cache_options):
        """What every constructor sets, after nn.Module's own: cache_options are what the generator asks of
        BaseDecoder.empty_cache / make_cache."""
        self.model = model.module if multi_gpu else model
        self.max_tgt_len = max_tgt_len
        self.start_pos = BOS
        self.eos_id = eos_id
        self.graph = graph
        self.captures = 0      # graphs captured so far (graph=True on a CUDA model; 0 otherwise)
        self._graphs = {}      # key -> SimpleNamespace of static buffers and the captured step (insertion-ordered)
        self._keep_graph = False  # keep the captured hipGraph_t (tools/bench_greedy.py counts its nodes)
        self._cache_options = cache_options
        self.early_stop = bool(early_stop)
        self.poll_every = self.POLL_EVERY
        self.last_steps_run = None  # decode steps that ran in the last call
        self.last_replays = None    # decode steps issued in the last call (>= last_steps_run: parked ones store nothing)
        self._check_early_stop()
        self.constraints = constraints

    def _check_early_stop(self):
        if self.early_stop and self.eos_id is None:
            raise ValueError(f"{type(self).__name__}: early_stop=True needs an eos_id (without one no row ever finishes)")

    def _check_eval(self):
        if self.model.training:
            raise RuntimeError(f"{type(self).__name__}: inference only (the model is in training mode)")

    def _encode(self, data):
        """process_data + encode: the (B, S, E) memory that the steps attend to."""
        with torch.no_grad():
            self.model.process_data(data)
            return self.model.encode(data)[0]

    @property
    def constraints(self):
        """The active DecodingConstraints, or None. Assignable between calls: None and an inactive value are the same
        thing, no constraint step at all (the launches, the graph key and the captured graph of a generator built
        without the keyword); another active value gets a captured graph of its own."""
        return self._constraints

    @constraints.setter
    def constraints(self, constraints):
        if constraints is not None and not isinstance(constraints, DecodingConstraints):
            raise TypeError("constraints must be a DecodingConstraints or None")
        object.__setattr__(self, "_constraints", constraints if constraints is not None and constraints.active else None)

    # ---- the state of a call and the step that runs on it ----

    def _state(self, cache, return_logp=False):
        """The static buffers beside the cache: tokens, the step counter, the finished flags, the suppress list of the
        constraints and the early-stop latch's words {all_prev, steps_run, parked, reserved} (each None where the
        generator has none), then the generator's own (_own_state). return_logp: keep the log-probabilities too (the
        beam has none to keep)."""
        (R, T), dev = cache.pad.shape, cache.pad.device
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)
        e = SimpleNamespace(cache=cache, ys=z(R, T, dtype=torch.long), t_dev=z(1, dtype=torch.int32),
                            fin=z(R, dtype=torch.uint8) if self.FIN_WITHOUT_EOS or self.eos_id is not None else None,
                            suppress=None if self.constraints is None else self.constraints.suppress_tensor(dev),
                            stop=z(4, dtype=torch.int32) if self.early_stop else None, stop_host=None)
        self._own_state(e, z, bool(return_logp))
        return e

    def _own_state(self, e, z, return_logp):
        pass

    def _reset(self, e):
        """Step 0 of a new batch: BOS everywhere, no row finished. The self-attention cache needs no reset (rows above t
        are never read); the beam's ancestry table is cleared so that every entry stays a valid row."""
        e.ys.zero_()
        e.ys[:, 0] = self.start_pos
        for buf in (e.cache.pad, e.cache.head_pad, e.cache.anc, e.fin, e.stop):
            if buf is not None:
                buf.zero_()
        e.t_dev.zero_()
        self._own_reset(e)

    def _own_reset(self, e):
        pass

    def _device_step(self, e):
        """One decode step with every step-dependent index read from e.t_dev (on the device where the kernels run): the
        same launches for every t, so they can be captured once. A finished row takes PAD (the beam: offers (cum, PAD))
        whatever its logits, so the constraints leave it alone. Ends by advancing the counter, after its last reader."""
        m = self.model
        x = m.tgt_embedding.step(e.ys, e.t_dev)
        dec = m.decoder.step(x, e.cache, e.t_dev)
        logits = m.generator.linear(dec[:, 0])
        if self.constraints is not None:
            self.constraints.apply(logits, e.ys, e.t_dev, fin=e.fin, suppress=e.suppress)
        self._select(e, logits)
        self._advance(e)

    def _advance(self, e):
        """The end of a device step, after the counter's last reader: the increment, or the early-stop latch."""
        if e.stop is None:
            e.t_dev.add_(1)
        else:
            from .decode_ops import decode_advance
            decode_advance(e.fin, e.t_dev, e.stop, self.max_tgt_len)

    def _run_steps(self, e, graphed, after_step=None):
        """The decode steps of one call on the reset state e: replays of e.graph (graphed) or eager _device_step calls,
        max_tgt_len - 1 of them or, with early_stop, until the latch reports parked (see the class docstring).
        after_step() runs on the host after each issued step. Sets last_steps_run and last_replays."""
        self._check_early_stop()
        n = self.max_tgt_len - 1
        step = e.graph.replay if graphed else (lambda: self._device_step(e))
        if e.stop is None:
            for _ in range(n):
                step()
                if after_step is not None:
                    after_step()
            self.last_steps_run = self.last_replays = n
            return
        issued = 0
        if not graphed:  # host-bound already: read the latch after every step
            while issued < n:
                step()
                issued += 1
                if after_step is not None:
                    after_step()
                if int(e.stop[2]) != 0:
                    break
            self.last_steps_run, self.last_replays = int(e.stop[1]), issued
            return
        poll = max(1, int(self.poll_every))
        chunks = (n + poll - 1) // poll
        if e.stop_host is None or e.stop_host.shape[0] < chunks + 1:
            e.stop_host = torch.empty(chunks + 1, 4, dtype=torch.int32, pin_memory=True)
        stream = torch.cuda.current_stream(e.stop.device)
        events = []
        while issued < n:
            k = len(events)
            if k >= 2:  # chunks k - 1 and k - 2 are in flight: wait for the older one's state words
                events[k - 2].synchronize()
                if int(e.stop_host[k - 2, 2]) != 0:
                    break
            for _ in range(min(poll, n - issued)):
                step()
                issued += 1
                if after_step is not None:
                    after_step()
            e.stop_host[k].copy_(e.stop, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            events.append(ev)
        e.stop_host[chunks].copy_(e.stop, non_blocking=True)
        stream.synchronize()
        self.last_steps_run, self.last_replays = int(e.stop_host[chunks, 1]), issued

    # ---- one reset state per call: a captured entry, or a fresh eager one ----

    def _prepare(self, enc, src_mask, return_logp=False):
        """(e, graphed) for the memory enc (B, S, E) and its key-padding mask: the captured entry with graph=True on a
        CUDA memory, otherwise a fresh cache and state; reset to step 0 either way."""
        return_logp = bool(return_logp)
        if self.graph and enc.is_cuda:
            return self._graph_entry(enc, src_mask, return_logp), True
        e = self._state(self.model.decoder.make_cache(enc, src_mask, self.max_tgt_len, **self._cache_options), return_logp)
        self._reset(e)
        return e, False

    def _key_extras(self):
        """The generator's own settings that a captured step holds as constants."""
        return ()

    def _constraint_key(self):
        """What the constraints add to the graph key: nothing when there are none."""
        return () if self.constraints is None else (self.constraints,)

    def _graph_key(self, enc, return_logp):
        """Reallocated parameters recapture; weights updated in place are simply read by the next replay. eos_id and
        early_stop add nothing when they are off."""
        m = self.model
        params = [p for mod in (m.tgt_embedding, m.decoder, m.generator.linear)
                  for p in list(mod.parameters()) + list(mod.buffers())]
        return (enc.device, enc.size(0), enc.size(1), self.max_tgt_len, *self._key_extras(), return_logp,
                *self._constraint_key(), *(() if self.eos_id is None else ("eos", int(self.eos_id))),
                *(("early_stop",) if self.early_stop else ()), tuple(p.data_ptr() for p in params))

    def _graph_entry(self, enc, src_mask, return_logp):
        """The captured entry for this memory (captured now if there is none, the oldest evicted), its static memory
        buffers loaded from enc and src_mask and its state reset to step 0: ready for max_tgt_len - 1 replays."""
        key = self._graph_key(enc, return_logp)
        e = self._graphs.get(key)
        if e is None:
            with torch.cuda.device(enc.device):
                e = self._capture(enc, return_logp)
            while len(self._graphs) >= self.MAX_GRAPHS:
                del self._graphs[next(iter(self._graphs))]
            self._graphs[key] = e
        self.model.decoder.load_memory(e.cache, enc, src_mask)
        self._reset(e)
        return e

    def _check_capture(self, enc):
        """Raises where the generator's own step cannot be captured for this memory."""

    def _capture(self, enc, return_logp):
        from ._lib import lib
        self._check_capture(enc)
        if self.constraints is not None and (not lib().csa_constrain_rows_supported(self.max_tgt_len)
                                             or enc.dtype != torch.float32):
            raise ValueError(f"{type(self).__name__}: graph=True with constraints needs fp32 and max_tgt_len <= 1024 "
                             "(csa_constrain_rows_supported)")
        dev = enc.device
        cache = self.model.decoder.empty_cache(enc.size(0), self.max_tgt_len, dev, enc.dtype, S=enc.size(1),
                                               **self._cache_options)
        e = self._state(cache, return_logp)
        self._reset(e)
        # one eager device-stepped step on a side stream first: code objects, hipBLASLt heuristics and workspaces
        # are then in place and stay outside the capture
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._device_step(e)
        torch.cuda.current_stream(dev).wait_stream(side)
        e.graph = torch.cuda.CUDAGraph(keep_graph=True) if self._keep_graph else torch.cuda.CUDAGraph()
        with torch.cuda.graph(e.graph):  # a single capture stream: the captured step has no parallel branches
            self._device_step(e)
        if self._keep_graph:
            e.graph.instantiate()
        self.captures += 1
        return e


class CachedGreedyGenerator(_SteppedDecoding, GreedyGenerator):
    """GreedyGenerator with a key/value cache: the same tokens from one decoder pass per NEW position.

    The decoder is causal and the key-padding mask of positions <= j never changes as ys grows, so step t needs only
    position t: its embedding, BaseDecoder.step against the cached self-attention keys / values and the once-projected
    encoder memory (csa_decode_attn), the Generator's linear on the B last rows, and the row argmax written into
    ys[:, t+1] with the next step's PAD byte (csa_argmax_rows). Eval-mode log(softmax(z)) is monotone in z, so the
    argmax of the logits is the reference's torch.max(out, 1)[1] and the softmax is skipped unless return_logp asks for
    the (max_tgt_len-1, B, V) last-position log-probabilities. All max_tgt_len-1 steps run, as in the reference, unless
    early_stop asks otherwise (below). In training mode this defers to GreedyGenerator.

    graph=True (eval mode, CUDA model): the loop above is bound by the host, about 70 small launches per step issued
    from Python. The step is instead run device-stepped (csa_decode_embed, csa_decode_attn_step, csa_argmax_rows_step)
    and replayed from one captured graph per (..., return_logp, ...) (_SteppedDecoding); process_data, encode (its
    Philox key comes from the CPU generator) and the memory projections stay eager. Same ids and log-probabilities,
    bitwise.

    constraints=DecodingConstraints(...): the logits of every step go through decode_ops.constrain_rows before the
    argmax (history = the row's tokens so far, BOS included; there is no finished flag here, so the rules keep applying
    after an EOS), and return_logp reports the constrained distribution. Training mode with active constraints
    raises: the uncached loop it defers to has no such step.

    eos_id (default None: the behaviour above, bit for bit): the generator keeps a finished flag per row, fin (B,) uint8.
    A row that has emitted eos_id takes PAD from then on (csa_argmax_rows_fin_step) and active constraints leave it
    alone. With the head-repeated PAD mask a finished row's PAD columns enter other rows' masks, so this is a behaviour
    of its own, not a truncation of the ids without eos_id. early_stop=True (needs eos_id; _SteppedDecoding) stops the
    call once every row has finished, with the ids of the full run, and return_logp then returns the steps that ran,
    (last_steps_run, B, V). Training mode with an eos_id raises."""

    FIN_WITHOUT_EOS = False

    def __init__(self, model, max_tgt_len, multi_gpu=False, graph=False, constraints=None, eos_id=None,
                 early_stop=False):
        super().__init__(model, max_tgt_len, multi_gpu)
        self._init_stepped(model, max_tgt_len, multi_gpu, eos_id, graph, early_stop, constraints,
                           repeat_heads=True)  # as CSATrans.decode masks

    def forward(self, data, return_logp=False):
        m = self.model
        if m.training:
            if self.constraints is not None or self.eos_id is not None:
                raise RuntimeError("CachedGreedyGenerator: constraints and eos_id are for inference only (the uncached "
                                   "loop that training mode defers to has neither)")
            ys = super().forward(data)
            self.last_steps_run = self.last_replays = self.max_tgt_len - 1
            return (ys, None) if return_logp else ys
        from .decode_ops import argmax_rows
        from .gen_ops import gen_log_softmax
        enc = self._encode(data)
        with torch.no_grad():
            if (self.graph and enc.is_cuda) or self.eos_id is not None:  # the device-stepped step, captured or eager
                return self._decode(*self._prepare(enc, data.src_mask, return_logp))
            # the host-stepped loop: an int step, csa_argmax_rows and csa_decode_attn
            B, T = enc.size(0), self.max_tgt_len
            cache = m.decoder.make_cache(enc, data.src_mask, T, **self._cache_options)
            ys = torch.zeros(B, T, dtype=torch.long, device=enc.device)
            ys[:, 0] = self.start_pos
            logps = []
            con = self.constraints
            suppress = None if con is None else con.suppress_tensor(enc.device)
            for t in range(T - 1):
                x = m.tgt_embedding.step(ys[:, t:t + 1], t)
                dec = m.decoder.step(x, cache, t)
                logits = m.generator.linear(dec[:, 0])
                if con is not None:
                    con.apply(logits, ys, t, suppress=suppress)
                argmax_rows(logits, out=ys[:, t + 1], is_pad=cache.pad[:, t + 1], pad_id=PAD)
                if return_logp:
                    logps.append(gen_log_softmax(logits, 0.0))
            self.last_steps_run = self.last_replays = T - 1
            out = ys[:, 1:]
            return (out, torch.stack(logps)) if return_logp else out

    def _own_state(self, e, z, return_logp):
        """The slot where each step leaves its log-probabilities when return_logp asks for them."""
        e.logp, e.return_logp = None, return_logp

    def _select(self, e, logits):
        from .decode_ops import argmax_rows
        from .gen_ops import gen_log_softmax
        # e.fin is None exactly when eos_id is: csa_argmax_rows_step, else csa_argmax_rows_fin_step
        argmax_rows(logits, out=e.ys, is_pad=e.cache.pad, pad_id=PAD, t_dev=e.t_dev, head_pad=e.cache.head_pad,
                    fin=e.fin, eos_id=self.eos_id)
        e.logp = gen_log_softmax(logits, 0.0) if e.return_logp else None

    def _decode(self, e, graphed):
        """The steps of one call on the reset state e; each step's log-probabilities are copied out of their slot as
        the step is issued, and those of the steps that ran are returned."""
        logps = []
        self._run_steps(e, graphed, (lambda: logps.append(e.logp.clone())) if e.return_logp else None)
        out = e.ys[:, 1:].clone()
        return (out, torch.stack(logps[:self.last_steps_run])) if e.return_logp else out


class BeamSearchGenerator(_SteppedDecoding, nn.Module):
    """Beam search of width W = beam_size over the KV-cached, device-stepped decode step (no counterpart in the
    reference, whose only strategy is GreedyGenerator).

    Rows are R = B * W hypotheses, row r = b * W + w. All max_tgt_len - 1 steps run (static shapes) unless
    early_stop=True (_SteppedDecoding) ends the call once every hypothesis has finished; the result is bitwise the same.
    cum (fp32) starts at 0 for row b * W and -inf for the other W - 1 rows, all tokens BOS. Per step the eval-mode
    generator logits z give logp = z - lse (fp32) and a candidate scores cum[r] + (z - lse[r]); a hypothesis that has
    emitted eos_id is finished (None: never), offers the single candidate (cum, PAD), and its row still runs through
    the decoder, ignored. Per AST the best W candidates survive: score descending, then parent row, then token.
    The self-attention key mask is the hypothesis' own PAD columns (make_std_mask per row, DecodeCache without
    repeat_heads): the reference decode()'s `.repeat(num_heads, 1, 1)` would let a finished hypothesis' padding mask
    keys of live ones, so it is not reproduced here.

    Nothing is gathered between steps: the K/V cache stays where each step stored it and the attention follows the
    (R, T) ancestry table that the selection rewrites (decode_ops.beam_row_topk / beam_select, decode_attention's anc=
    and kv_group=); the W hypotheses of an AST share one memory projection. The step index lives in a 4-byte device
    counter, so the launches of a step never depend on it.

    After the last step the W hypotheses of an AST are ranked by cum / len ** length_penalty, len counting tokens up
    to and including the first EOS (max_tgt_len - 1 without one). forward returns the best ids (B, max_tgt_len - 1),
    PAD after EOS; with return_all also the ids (B, W, max_tgt_len - 1) and scores (B, W) in rank order.

    graph=True (CUDA model): as CachedGreedyGenerator, the step is replayed from one captured graph per
    (..., beam_size, ...) (_SteppedDecoding); bitwise the eager result. Inference only: a model in training mode
    raises.

    constraints=DecodingConstraints(...): every live hypothesis' logits go through decode_ops.constrain_rows (its own
    history, as the selection rewrote it) before the row top-W; a banned token is a -inf logit, so lse and the scores
    are those of the distribution renormalised over what is left. Finished hypotheses are left alone."""

    def __init__(self, model, max_tgt_len, beam_size, length_penalty=0.0, eos_id=EOS, multi_gpu=False, graph=False,
                 constraints=None, early_stop=False):
        super().__init__()
        if not 1 <= beam_size <= 8:
            raise ValueError("BeamSearchGenerator: beam_size must be in [1, 8]")
        if max_tgt_len < 2:
            raise ValueError("BeamSearchGenerator: max_tgt_len must be at least 2")
        self.beam_size = beam_size
        self.length_penalty = float(length_penalty)
        self._init_stepped(model, max_tgt_len, multi_gpu, eos_id, graph, early_stop, constraints, beam=beam_size)

    def forward(self, data, return_all=False):
        self._check_eval()
        return self.search(self._encode(data), data.src_mask, return_all)

    def search(self, enc, src_mask=None, return_all=False):
        """The decoder side alone: enc (B, S, E) batch-first memory (any source, CPU included), src_mask (B, S) bool
        key-padding mask or None."""
        self._check_eval()
        V = self.model.generator.linear.weight.shape[0]
        if V < self.beam_size:
            raise ValueError("BeamSearchGenerator: the target vocabulary is smaller than the beam")
        with torch.no_grad():
            e, graphed = self._prepare(enc, src_mask)
            self._run_steps(e, graphed)
            return self._rank(e, enc.size(0), return_all)

    def _key_extras(self):
        return (self.beam_size,)

    def _own_state(self, e, z, return_logp):
        """Per hypothesis the cumulative log-probability, and the row top-W buffers between the two kernels."""
        R, W = e.ys.shape[0], self.beam_size
        e.cum, e.lse = z(R, dtype=torch.float32), z(R, dtype=torch.float32)
        e.topv, e.topi = z(R, W, dtype=torch.float32), z(R, W, dtype=torch.int32)

    def _own_reset(self, e):
        """One live hypothesis per AST."""
        e.cum.fill_(float("-inf"))
        e.cum.view(-1, self.beam_size)[:, 0] = 0.0

    def _select(self, e, logits):
        from .decode_ops import beam_row_topk, beam_select
        beam_row_topk(logits, self.beam_size, e.lse, e.topv, e.topi, t_dev=e.t_dev, t_end=self.max_tgt_len - 1)
        beam_select(e.topv, e.topi, e.lse, e.cum, e.fin, e.ys, e.cache.pad, e.cache.anc, e.t_dev, eos_id=self.eos_id,
                    pad_id=PAD)

    def _rank(self, e, B, return_all):
        W, T = self.beam_size, self.max_tgt_len
        ids = e.ys[:, 1:]
        length = torch.full((B * W,), T - 1, dtype=torch.long, device=ids.device)
        if self.eos_id is not None:
            is_eos = ids == self.eos_id
            length = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, length)
        score = e.cum.clone() if self.length_penalty == 0.0 else e.cum / length.float() ** self.length_penalty
        score = score.view(B, W)
        order = torch.argsort(score, dim=1, descending=True, stable=True)
        ranked = ids.reshape(B, W, T - 1).gather(1, order[:, :, None].expand(B, W, T - 1))
        best = ranked[:, 0].clone()
        return (best, ranked, score.gather(1, order)) if return_all else best

    def _check_capture(self, enc):
        from ._lib import lib
        if not lib().csa_beam_supported(self.beam_size, self.max_tgt_len) or enc.dtype != torch.float32:
            raise ValueError("BeamSearchGenerator: graph=True needs fp32 and max_tgt_len <= 256 (csa_beam_supported)")


class SamplingGenerator(_SteppedDecoding, nn.Module):
    """Sampled decoding over the KV-cached, device-stepped decode step: num_samples independent draws per AST from the
    model's distribution, filtered by temperature, top_k (0: off) and top_p (>= 1: off), with the log-probability of
    every drawn token (no counterpart in the reference, whose only strategy is GreedyGenerator).

    Rows are R = B * num_samples, row r = b * num_samples + s. Each row keeps its own self-attention cache row (no
    ancestry table); the rows of an AST share one memory projection and mask (DecodeCache kv_group, make_cache's
    group=). The self-attention key mask is the row's own PAD columns, as in BeamSearchGenerator and for its reason:
    the reference decode()'s `.repeat(num_heads, 1, 1)` would let a finished sample's padding mask keys of live ones.
    Per step the eval-mode generator logits go through decode_ops.sample_rows (csrc/csa_sample.hip): y = z /
    temperature, top-k with all ties, top-p on the renormalised top-k set (tie-inclusive), one Gumbel-max draw from
    Philox stream 7 keyed by (seed, row, step, column), logp = y[token] - lse(y over the kept set). A row that has
    emitted eos_id is finished (None: never): it takes PAD with logp 0 and still runs through the decoder, ignored.
    All max_tgt_len - 1 steps run (static shapes) unless early_stop=True (_SteppedDecoding) ends the call once every row
    has finished; ids and log-probabilities are bitwise the same.

    forward(data, seed=None, return_logp=False) / sample(enc, src_mask, seed, return_logp) return the ids
    (B, max_tgt_len - 1), or (B, num_samples, max_tgt_len - 1) when num_samples > 1, PAD after EOS; with return_logp
    also the per-token log-probabilities of the same shape, 0 after EOS, whose sum over the last dim is the sequence
    log-probability under the sampled (filtered) distribution. seed: a 64-bit key; None draws one from torch's CPU
    generator (reproducible under torch.manual_seed). The same seed repeats the same draws on any device path.

    graph=True (CUDA model): as CachedGreedyGenerator, the step is replayed from one captured graph per
    (..., temperature, top_k, top_p, num_samples, eos_id, return_logp, ...) (_SteppedDecoding); the seed lives in a
    16-byte device buffer filled outside the graph, so a replay draws anew. Bitwise the eager result. Inference only:
    a model in training mode raises.

    constraints=DecodingConstraints(...): every live row's logits go through decode_ops.constrain_rows before
    sample_rows, which never draws a -inf entry and renormalises: logp is the log-probability under the constrained,
    filtered distribution. Finished rows are left alone."""

    def __init__(self, model, max_tgt_len, temperature=1.0, top_k=0, top_p=1.0, num_samples=1, eos_id=EOS,
                 multi_gpu=False, graph=False, constraints=None, early_stop=False):
        super().__init__()
        if not float(temperature) > 0.0:
            raise ValueError("SamplingGenerator: temperature must be positive")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError("SamplingGenerator: top_k must be a non-negative integer (0 turns it off)")
        if not float(top_p) > 0.0:
            raise ValueError("SamplingGenerator: top_p must be positive (1 or more turns it off)")
        if int(num_samples) != num_samples or num_samples < 1:
            raise ValueError("SamplingGenerator: num_samples must be a positive integer")
        if max_tgt_len < 2:
            raise ValueError("SamplingGenerator: max_tgt_len must be at least 2")
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.num_samples = int(num_samples)
        self._init_stepped(model, max_tgt_len, multi_gpu, eos_id, graph, early_stop, constraints,
                           group=self.num_samples)

    def forward(self, data, seed=None, return_logp=False):
        self._check_eval()
        return self.sample(self._encode(data), data.src_mask, seed, return_logp)

    def sample(self, enc, src_mask=None, seed=None, return_logp=False):
        """The decoder side alone: enc (B, S, E) batch-first memory (any source, CPU included), src_mask (B, S) bool
        key-padding mask or None."""
        self._check_eval()
        if seed is None:  # one 64-bit Philox key per call from torch's global CPU generator, as ops._draw_seed
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        key = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed, 0], dtype=torch.int64)  # {seed, offset}
        with torch.no_grad():
            e, graphed = self._prepare(enc, src_mask, return_logp)
            e.rng.copy_(key)  # outside the graph: the replays read it on the device
            self._run_steps(e, graphed)
            B, S, T = enc.size(0), self.num_samples, self.max_tgt_len
            shape = (B, T - 1) if S == 1 else (B, S, T - 1)
            ids = e.ys[:, 1:].reshape(shape).clone()
            return (ids, e.logp.reshape(shape).clone()) if return_logp else ids

    def _key_extras(self):
        return (self.temperature, self.top_k, self.top_p, self.num_samples)

    def _own_state(self, e, z, return_logp):
        """The {seed, offset} key that the kernel reads on the device and, when asked for, the per-token
        log-probabilities."""
        R, T = e.ys.shape
        e.rng = z(2, dtype=torch.int64)
        e.logp = z(R, T - 1, dtype=torch.float32) if return_logp else None

    def _own_reset(self, e):
        if e.logp is not None:
            e.logp.zero_()

    def _select(self, e, logits):
        from .decode_ops import sample_rows
        sample_rows(logits, e.ys, e.cache.pad, e.fin, e.t_dev, e.rng, temperature=self.temperature, top_k=self.top_k,
                    top_p=self.top_p, eos_id=self.eos_id, pad_id=PAD, logp=e.logp)

    def _check_capture(self, enc):
        from ._lib import lib
        if not lib().csa_sample_rows_supported(self.model.generator.linear.weight.shape[0]) or enc.dtype != torch.float32:
            raise ValueError("SamplingGenerator: graph=True needs fp32 and a target vocabulary of at most 32768 "
                             "(csa_sample_rows_supported)")
