"""SalmonnRuntime — the MI355X-native stand-in for the external ``SALMONN.models.salmonn_org.SALMONN``
object that the reference builds at models/custom_salmon.py:96 and drives through
``encode_speech`` (:550), ``llama_model(...)`` (:631) and ``llama_model.generate(...)`` (:705).

It owns the packed weights (HBM resident, bf16), one ``Workspace`` of activation buffers and the four
kernel chains of runtime/engines.py.  Prompts arrive as *segments* (token-id runs and speech-row runs)
so that the string work of ``custom_prompt_wrap`` stays on the host while the interleave itself is one
gather kernel (K9).  Everything arithmetic goes through libicl_hip; there is no CPU fallback.
"""
from __future__ import annotations

import gc
import os

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import binding as B
from . import probes as P
from .config import SalmonnCfg
from .engines import BF16, F32, I32, BeatsHIP, KVCache, LlamaHIP, LogMel, SpeechQFormerHIP, WhisperEncoderHIP, Workspace, _i32, check_kv_dtype
from .packing import normalize_keys, pack_beats, pack_llama, pack_qformer, pack_whisper

Segment = Union[Sequence[int], Tuple[str, int, int]]  # token ids | ("speech", first_row, n_rows)


def speech_segment(first_row: int, n_rows: int) -> Tuple[str, int, int]:
    return ("speech", first_row, n_rows)


@dataclass
class GenerateResult:
    tokens: torch.Tensor          # int64 [B, width] on CPU — what HF generate() returns with inputs_embeds
    first_logits: Optional[torch.Tensor] = None  # f32 [B, V] (device) logits of the first generated position
    step_logits: Optional[torch.Tensor] = None   # f32 [max_new_tokens, B, V] (device): the logits every token was chosen from
    dropped: Tuple[int, ...] = ()                # rows NOT generated (``overlong="drop"``): pad-filled tokens, NaN logits
    token_logprobs: Optional[torch.Tensor] = None   # f32 [B, width] on CPU, with a ``constraint`` only: log-probability of every
    #                                                 token among the candidates it was chosen from (0 after a row's EOS)
    hidden = None    # or f32 [B, n_layers + 1, hidden] (device), with ``want_hidden``: the residual stream of the last prompt row at
    #                  every site, pre-patch at a patched site.  An attribute set after construction, not a dataclass field: the
    #                  fields are what a result of a plain call consists of (the pinned generate trace lists them)
    head_out = None  # or bf16 [B, n_layers, n_heads, head_dim] (device), with ``want_heads``: the head outputs of the last prompt row
    #                  in every layer, as o_proj would have read them, pre-patch.  Set after construction, like ``hidden``


@dataclass
class PromptAttention:
    """``prompt_attention``: where the prompt's last row — the query that decides the first generated token — looks."""
    mass: torch.Tensor                  # f32 [B, n_layers, n_heads, n_seg] on CPU: attention mass per segment of the prompt
    probs: Optional[torch.Tensor]       # None, or f32 [B, n_layers, n_heads, max_len] (device); row b is valid up to lens[b]
    first_logits: torch.Tensor          # f32 [B, V] (device): generate(..., want_first_logits=True).first_logits, bit for bit
    lens: List[int]                     # prompt lengths (positions)
    flow = None      # or f32 [B, n_layers, n_heads, n_seg, n_seg] on CPU, with ``want_flow``: the attention mass EVERY query row of
    #                  segment a sends to the keys of segment c, summed over the rows (``flow / rows[:, None, None, :, None]``: the mean)
    rows = None      # or int64 [B, n_seg] on CPU, with ``want_flow``: the positions of every segment.  Both are attributes set after
    #                  construction, not dataclass fields: the fields are what a result of a plain call consists of (pinned trace)


def _undrop(sub: GenerateResult, keep: List[int], bad: List[int], n: int, pad: int) -> GenerateResult:
    """``overlong="drop"``: the result of the kept rows scattered back to ``n`` rows; a dropped row's tokens are pad, its logits
    and log-probabilities NaN."""
    def spread(x, dim, fill):
        if x is None:
            return None
        shape = list(x.shape)
        shape[dim] = n
        out = torch.full(shape, fill, dtype=x.dtype, device=x.device)
        out[(slice(None),) * dim + (torch.tensor(keep).to(x.device),)] = x
        return out
    nan = float("nan")
    res = GenerateResult(tokens=spread(sub.tokens, 0, pad), first_logits=spread(sub.first_logits, 0, nan),
                         step_logits=spread(sub.step_logits, 1, nan), dropped=tuple(bad),
                         token_logprobs=spread(sub.token_logprobs, 0, nan))
    if sub.hidden is not None:
        res.hidden = spread(sub.hidden, 0, nan)
    if sub.head_out is not None:
        res.head_out = spread(sub.head_out, 0, nan)
    return res


def _is_speech(seg) -> bool:
    return isinstance(seg, tuple) and len(seg) == 3 and seg[0] == "speech"


class CausalLMRuntimeMixin:
    """K9-K12 over a packed decoder (`self.llama`: LlamaHIP, `self.lm_cfg`: LlamaCfg, `self.ws`, `self.device`):
    prompt segments -> gather/interleave -> prefill -> greedy decode / teacher-forced logits.  Shared by the SALMONN
    (Llama-2 / Vicuna) and Qwen2-Audio runtimes."""

    use_graphs = True          # capture the decode loop in a HIP graph (per batch shape) after its first eager pass
    kv_dtype = "bf16"          # the decoder's KV cache: "bf16", or "fp8" (the opt-in FP8 KV cache; engines.KVCache)

    # --------------------------------------------------------------------------------------------
    # K9: prompt segments -> gather indices
    # --------------------------------------------------------------------------------------------
    def _gather_indices(self, prompts: Sequence[Sequence[Segment]], n_speech_rows: int) -> Tuple[List[int], List[int]]:
        V = self.lm_cfg.vocab
        flat: List[int] = []
        lens: List[int] = []
        for segs in prompts:
            before = len(flat)
            for seg in segs:
                if _is_speech(seg):
                    _, first, cnt = seg
                    if first < 0 or first + cnt > n_speech_rows:
                        raise ValueError(f"speech segment [{first},{first + cnt}) outside {n_speech_rows} speech rows")
                    flat.extend(-(r + 1) for r in range(first, first + cnt))
                else:
                    for t in seg:
                        t = int(t)
                        if not 0 <= t < V:
                            raise ValueError(f"token id {t} outside the vocabulary [0,{V})")
                        flat.append(t)
            if len(flat) == before:
                raise ValueError("empty prompt")
            lens.append(len(flat) - before)
        return flat, lens

    @staticmethod
    def _prompt_lengths(prompts: Sequence[Sequence[Segment]]) -> List[int]:
        """Positions per prompt (host arithmetic only; the validation of ``generate`` runs before anything is launched)."""
        return [sum(seg[2] if _is_speech(seg) else len(seg) for seg in segs) for segs in prompts]

    def embed_prompts(self, prompts, speech: Optional[torch.Tensor], name: str = "ll_h"):
        rows = 0 if speech is None else speech.shape[0] * (speech.shape[1] if speech.dim() == 3 else 1)
        sp2 = None if speech is None else speech.reshape(rows, self.lm_cfg.hidden).contiguous()
        flat, lens = self._gather_indices(prompts, rows)
        h = self.llama.embed(self.ws, _i32(flat, self.device), sp2, name=name)
        return h, lens

    # --------------------------------------------------------------------------------------------
    # K10 (+K12): teacher-forced forward
    # --------------------------------------------------------------------------------------------
    def forward_logits(self, prompts, speech: Optional[torch.Tensor]) -> Tuple[torch.Tensor, List[int]]:
        """All-position logits f32 [sum S_b, V] (packed) and the per-sequence lengths."""
        h, lens = self.embed_prompts(prompts, speech, name="fw_h")
        self.llama.prefill(self.ws, h, lens, cache=None)
        return self.llama.logits(self.ws, h, name="fw_logits"), lens

    def cross_entropy(self, logits: torch.Tensor, shifted_labels: torch.Tensor) -> torch.Tensor:
        """mean CE over rows with label >= 0; logits f32 [M, V] (device), shifted_labels int32 [M]."""
        M = logits.shape[0]
        rows = self.ws.get("ce_rows", (M,), F32)
        mean = self.ws.get("ce_mean", (1,), F32)
        B.cross_entropy(logits, shifted_labels.to(device=self.device, dtype=I32), rows, mean)
        return mean

    # ---- K10 + K11: generate — first the pieces that the greedy / sampled / constrained search and beam search share ----
    MAX_GRAPHS = 16            # captured decode graphs kept (one per batch shape / cache length / knob set); oldest dropped
    prefill_chunk = int(os.environ.get("ICL_PREFILL_CHUNK", "128"))   # sequences per prefill pass (``_prefill_logits``)
    beam_rows = 256            # decode rows (sequences x beams) per pass of beam search: the widest decode tile

    def _cache(self, n_seqs: int, max_len: int) -> KVCache:
        """K/V views over the workspace's one K and one V allocation (they grow to the largest n_seqs x max_len seen; a
        move bumps ``ws.generation``, which retires every captured graph)."""
        return KVCache(self.lm_cfg, n_seqs, max_len, self.ws, dtype=self.kv_dtype)

    def _cache_len(self, lens: List[int], max_new_tokens: int, multiple: int) -> int:
        need = max(lens) + max_new_tokens
        max_len = -(-need // multiple) * multiple
        assert max_len <= self.lm_cfg.max_pos, f"prompt + new tokens ({need}) exceeds max_pos {self.lm_cfg.max_pos}"  # validated
        return max_len

    def _prefill_logits(self, h, lens: List[int], cache: KVCache, last, probes: Optional[P.Probes] = None) -> torch.Tensor:
        """Prefill in chunks of at most ``prefill_chunk`` sequences (the caller decodes ALL of them together: the decode GEMMs
        stream the weights once per step whatever the row count — 256 rows cost 0.84 us each against 1.06 at 128 — while the
        prefill GEMMs measured 1.3 % faster per utterance at 128 sequences than at 256; a sequence's arithmetic does not depend
        on its neighbours in either phase, so the split changes no result).  Only the last position of every prompt is read
        afterwards: the prefill writes those rows into ``last`` f32 [n, hidden] and trims its last layer to them
        (LlamaHIP.prefill, last_rows_only).  ``probes``: each chunk gets its rows of them (None: a chunk that lists no row
        launches as ever).  Returns their logits, f32 [n, vocab]."""
        r0 = 0
        for b0 in range(0, len(lens), self.prefill_chunk):
            b1 = min(len(lens), b0 + self.prefill_chunk)
            r1 = r0 + sum(lens[b0:b1])
            self.llama.prefill(self.ws, h[r0:r1], lens[b0:b1], cache.rows(b0, b1), last_rows_only=True, last_out=last[b0:b1],
                               probes=None if probes is None else probes.rows(b0, b1))
            r0 = r1
        return self.llama.logits(self.ws, last, name="gen_logits")

    def _step_tables(self, lens: List[int], steps: int):
        """(position of the fed token, cache length after its append, sequence id) of every decode row — ``lens`` = its
        prompt length — for each of ``steps`` decode steps: static buffers, so a captured graph can replay over them."""
        ws, n = self.ws, len(lens)
        pos_all, len_all, sid = ws.get("gen_pos", (steps, n), I32), ws.get("gen_len", (steps, n), I32), ws.get("gen_sid", (n,), I32)
        pos_all.copy_(torch.tensor([[s + t for s in lens] for t in range(steps)], dtype=I32), non_blocking=True)
        len_all.copy_(torch.tensor([[s + t + 1 for s in lens] for t in range(steps)], dtype=I32), non_blocking=True)
        sid.copy_(torch.arange(n, dtype=I32), non_blocking=True)
        return pos_all, len_all, sid

    def _graph_reset(self) -> None:
        """No captured decode graph and no warm key, as of the workspace's current generation."""
        self._graphs, self._graph_warm, self._graph_gen = {}, set(), self.ws.generation

    def _run_decode(self, gkey, decode_loop) -> None:
        """Enqueue ``decode_loop()``.  It is launch-bound at small batch (~17 kernels x layers x steps), so with ``use_graphs``
        a key's first call runs it eagerly (which sizes every workspace buffer), the second captures it into a HIP graph and
        replays that, later ones replay — all pointers are workspace-stable and nothing inside synchronises or allocates.  A
        graph bakes raw pointers into workspace buffers: a move (``ws.generation``) retires every graph and warm key.  The
        garbage collector is off inside the capture: a dead reference cycle may hold GPU objects (another runtime's graphs,
        events, buffers) whose finalisers make HIP calls that a capturing stream does not allow — the process aborts."""
        if not self.use_graphs:
            return decode_loop()
        if self._graph_gen != self.ws.generation:
            self._graph_reset()
        graph = self._graphs.get(gkey)
        if graph is None and gkey not in self._graph_warm:
            decode_loop()
            if self._graph_gen != self.ws.generation:                # the eager pass may have grown buffers
                self._graph_reset()
            self._graph_warm.add(gkey)
            return
        if graph is None:
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            prof, B.GEMM_PROFILE = B.GEMM_PROFILE, None              # no timing events inside a stream capture
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph):
                    decode_loop()
            finally:
                B.GEMM_PROFILE = prof
                if gc_was_on:
                    gc.enable()
            while len(self._graphs) >= self.MAX_GRAPHS:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[gkey] = graph
        graph.replay()

    def _decode_tail(self, state, max_new_tokens: int, eos, pad: int, constraint, knobs, do_sample: bool, generator,
                     sample_debug):
        """``(tail, graph-key element, token log-probs | None)``: ``tail(logits, step)`` picks every row's token of one step
        into ``state`` = (finished, tokens, next ids) — ``icl_argmax_fsm`` with a ``constraint``, the sampling kernel with
        ``knobs`` = (temperature, top_k, top_p, repetition_penalty), else plain argmax.  Sets up the buffers only: every
        argument was validated by ``generate``."""
        c, ws = self.lm_cfg, self.ws
        finished, toks, nxt = state
        Bn = toks.shape[0]
        if constraint is not None:
            # the automaton's tables are uploaded once and kept; the rows' states restart from their start states on every call
            # (outside the captured decode loop, like ``finished``), and the upload's id keys the graph
            tables = constraint[0].upload(self.device)
            fsm_state = ws.get("gen_fsm_state", (Bn,), I32)
            fsm_state.copy_(torch.tensor(constraint[1], dtype=I32), non_blocking=True)
            lps = ws.get("gen_token_logprobs", (Bn, max_new_tokens), F32)
            return (lambda lg, step: B.argmax_fsm(lg, tables, fsm_state, max_new_tokens - step, eos, pad, finished, toks, step, nxt,
                                                  out_logprob=lps, V=c.vocab)), ("fsm", tables.uid), lps
        if knobs is None:
            return (lambda lg, step: B.argmax_eos(lg, eos, pad, finished, toks, step, nxt, V=c.vocab)), None, None
        uni = ws.get("gen_uniform", (max_new_tokens, Bn), F32)
        if do_sample and generator is not None and generator.device.type != uni.device.type:
            uni.copy_(torch.rand(uni.shape, generator=generator))      # a host generator: draw there, same stream of uniforms
        elif do_sample:
            uni.uniform_(0.0, 1.0, generator=generator)
        else:
            uni.zero_()
        work = ws.get("gen_sample_work", (Bn, c.vocab), F32)
        return (lambda lg, step: B.sample_eos(lg, work, uni[step], eos, pad, finished, toks, step, nxt, temperature=knobs[0],
                                              top_k=knobs[1], top_p=knobs[2], repetition_penalty=knobs[3], V=c.vocab,
                                              debug=sample_debug if step == 0 else None)), knobs, None

    def generate(self, prompts, speech: Optional[torch.Tensor], max_new_tokens: int = 10, eos_id: Optional[int] = None,
                 pad_id: Optional[int] = None, suppress_eos: bool = False, want_first_logits: bool = False,
                 cache_len_multiple: int = 64, do_sample: bool = False, temperature: float = 1.0, top_p: float = 1.0,
                 top_k: int = 50, repetition_penalty: float = 1.0, generator: Optional[torch.Generator] = None,
                 sample_debug=None, want_step_logits: bool = False, overlong: str = "raise", num_beams: int = 1,
                 length_penalty: float = 1.0, beam_debug: Optional[dict] = None, constraint=None,
                 knockout=None, want_hidden: bool = False, patch=None, want_heads: bool = False, head_patch=None,
                 cuts=None) -> GenerateResult:
        """Greedy search with HF ``generate(inputs_embeds=…)`` semantics (models/custom_salmon.py:704-720): returns only
        the new tokens; a row that has emitted EOS is filled with pad; the width is that of the longest row
        (``min_length`` is a no-op with inputs_embeds).  All steps are enqueued without a host sync; the
        early-stop width is applied on the host afterwards (identical output, no per-token round trip).

        ``do_sample=True`` switches the tail to the sampling kernel (HF's sample mode: repetition penalty → temperature →
        top-k → top-p → draw; ``temperature`` / ``top_p`` / ``top_k`` are ignored otherwise, as in HF); a repetition penalty
        ≠ 1 in greedy mode runs the same kernel with ``top_k = 1``.  The draws are uniforms from ``generator`` (a device
        generator; default: torch's global CUDA generator): reproducible for a seed, not bit-identical to
        ``torch.multinomial``.

        ``overlong``: a row whose prompt + ``max_new_tokens`` exceeds ``max_pos`` is validated on the host BEFORE any launch.
        ``"raise"`` (default) fails the call; ``"drop"`` generates the other rows and reports the row in ``dropped`` (its
        tokens are pad, its logits NaN) — the reference runs batch 1, where one over-long prompt costs one utterance
        (inference/inference.py:370-373), not the batch it happens to be collated with.

        ``num_beams > 1``: HF beam search (``early_stopping=False``; ``length_penalty`` as in HF; see ``_generate_beam``).

        ``constraint`` = ``(constraints.LabelAutomaton, start_states)``, one start state per prompt (-1 = a free row): opt-in
        label-constrained greedy decoding.  The tail of every step is ``icl_argmax_fsm``: a constrained row's token is the best
        of the outgoing edges of its automaton state that can still reach an accepting state within the tokens left, so a row
        that runs out of ``max_new_tokens`` stops on a complete answer; the result carries ``token_logprobs``.  Prefill, KV cache
        and decode step are the unconstrained ones.  Greedy only: sampling, a repetition penalty, beams and ``suppress_eos``
        together with a constraint, a ``max_new_tokens`` below a row's shortest answer, and a start-state list of the wrong
        length are ``ValueError``s raised before anything is launched.

        ``knockout`` = ``(segments, blocked, layers, heads)`` (the last two optional; or a dict with those keys): opt-in
        attention knockout, the causal companion of ``prompt_attention``.  ``segments[b]``: one id (0..255) per position of
        prompt b, as for the readout; ``blocked[b]``: the segment ids (0..31) row b may not read, empty = the row is not
        touched; ``layers``: a half-open range ``(l0, l1)`` of decoder layers (None: all); ``heads``: query-head indices (None:
        all).  In those layers and heads the query of the LAST prompt position of row b and of every generated position gives
        weight 0 to every key of a blocked segment, and the softmax runs over the rest (generated positions are always
        visible); every other query of the prompt sees what it always saw.  One more launch (icl_attn_decode_masked_bf16) per
        windowed layer, prefill chunk and decode step rewrites those rows of the attention output; rows with an empty set keep
        their bits, and a knockout whose every set is empty is no knockout.  Works with every tail above; ``ValueError`` before
        any launch: the FP8 KV cache, beams, a segment list of the wrong length, ids outside 0..255, a blocked id outside 0..31, a
        layer window outside ``[0, n_layers]`` or empty, a head index out of range, a row whose blocked set covers its whole
        prompt.

        ``want_hidden`` and ``patch``: the residual stream at the deciding rows, read and written.  A decoder of n_layers layers
        has n_layers + 1 sites: site l < n_layers is the f32 stream at the input of layer l, before its input norm (HF
        ``hidden_states[l]``), site n_layers the output of the last layer before the final norm.  ``want_hidden``: the result's
        ``hidden`` f32 [B, n_layers + 1, hidden] (device) holds the LAST prompt row at every site, pre-patch at a patched site
        (dropped rows: NaN); ``layer_logits`` turns it into the logit lens.  ``patch`` = a dict ``site``, ``vectors`` (f32, CPU or
        device: [B, hidden] one per prompt, or [1, hidden] / [hidden] shared), ``mode`` "replace" (default) | "add", ``alpha`` (1.0;
        add only: row += alpha * vector, one rounding), ``rows`` (None: all, or distinct prompt indices; an empty list is no
        patch), ``steps`` "prompt" (default: the last prompt row only) | "all" (every generated row as well).  One launch
        (icl_resid_rows_f32) per site and prefill chunk with ``want_hidden``, one per chunk with a patch alone, and with
        ``steps="all"`` one per decode step plus the patched layer's input norm as a launch of its own; rows not listed keep
        their bits.  Works with every tail above, both KV dtypes and both weight dtypes.  ``ValueError`` before any launch:
        unknown keys, a site outside 0..n_layers, vectors of the wrong shape or dtype, a bad mode or steps, a non-finite alpha,
        a duplicate or out-of-range row, beams, ``patch`` together with ``knockout``.

        ``want_heads`` and ``head_patch``: the output of single attention heads at the deciding rows — the head_dim-vector a head
        hands to o_proj — read and written.  ``want_heads``: the result's ``head_out`` bf16 [B, n_layers, n_heads, head_dim]
        (device) holds the LAST prompt row's head outputs in every layer, as o_proj would have read them (after a knockout's
        rewrite), before a head patch (dropped rows: NaN); ``head_contrib`` turns them into the heads' summands of the residual
        stream.  ``head_patch`` = a dict ``heads`` ([(layer, head), ...], distinct), ``vectors`` (f32, CPU or device: [B, n_pairs,
        head_dim] one block per prompt, or [n_pairs, head_dim] / [1, n_pairs, head_dim] shared, in the order of ``heads``), and
        ``mode``, ``alpha``, ``rows``, ``steps`` as for ``patch`` (replace: head = bf16(vector); add: head = bf16(fma(alpha,
        vector, head))).  One launch (icl_head_rows_bf16) per layer and prefill chunk with ``want_heads``; a patch alone launches
        only in the layers that hold a selected head and in the chunks that list a row, and with ``steps="all"`` once per such
        layer and decode step; the decode steps keep their form (the fused RoPE + attention launch writes the buffer too).  Heads
        not selected and rows not listed keep their bits.  Works with every tail above, both KV dtypes and both weight dtypes,
        grouped-query and QK-norm decoders.  ``ValueError`` before any launch: unknown keys, a pair outside [0, n_layers) x [0,
        n_heads) or given twice, vectors of the wrong shape or dtype, a bad mode or steps, a non-finite alpha, a duplicate or
        out-of-range row, beams (also for ``want_heads``), ``head_patch`` together with ``knockout`` or with ``patch``.

        ``cuts`` = a dict ``segments``, ``pairs``, and optionally ``layers``, ``heads``, ``generated``: opt-in attention cuts
        between prompt segments, the edges of an information-flow study whose QUERY is an interior prompt row.  ``segments`` as
        for the knockout; ``pairs``: one list of ``(q_seg, k_seg)`` (both 0..31) for all prompts, or one list per prompt;
        ``layers`` / ``heads`` as for the knockout.  In those layers and heads a query at prompt position p whose segment is q_seg
        attends as if every key j <= p of segment k_seg were absent — transformers' 4-D additive mask with -inf at row i, column
        j where j > i or seg[j] is cut for seg[i].  A generated row reads every generated key and queries under the pairs of
        ``generated`` (a segment id per prompt or one for all; None: the segment of the prompt's last position; an id >= 32 or
        one without pairs leaves the generated rows, the decode steps and their graph key the plain ones).  Position p is
        LISTED iff a key it could read is cut: one more launch (icl_attn_cut_rows_bf16) per windowed layer and prefill chunk
        rewrites the listed rows of the attention output from the rotated q and the bf16 cache, tiles of rows of one sequence
        sharing one pass over its K / V; rows not listed keep their bits, and cuts that list no row are no cuts.  In the
        model's last layer only the sequences' last rows are launched (no other row of that layer can influence anything:
        exact).  The decode steps use the knockout's launch.  Works with every tail above, ``want_hidden`` / ``want_heads``,
        grouped-query and QK-norm decoders.  ``ValueError`` before any launch: unknown keys, a segment list of the wrong number
        or length, ids outside 0..255, a pair id outside 0..31, a bad ``layers``, ``heads`` or ``generated``, beams, the FP8 KV
        cache, ``cuts`` together with ``knockout``, ``patch`` or ``head_patch``, a listed row left without a visible key."""
        args = {k: v for k, v in locals().items() if k not in ("self", "prompts", "speech")}   # the keyword arguments, as given
        c, ws = self.lm_cfg, self.ws
        # ---- 1. validate: every caller error is raised here, before anything is launched
        if overlong not in ("raise", "drop"):
            raise ValueError(f"overlong must be 'raise' or 'drop', not {overlong!r}")
        if constraint is not None:
            constraint = self._check_constraint(constraint, len(prompts), max_new_tokens, eos_id, do_sample, repetition_penalty,
                                                num_beams, suppress_eos)
        limit = c.max_pos // cache_len_multiple * cache_len_multiple      # cache lengths are multiples of cache_len_multiple
        plens = self._prompt_lengths(prompts)
        checked = P.check_probes(c, self.kv_dtype, plens, num_beams, knockout=knockout, patch=patch, head_patch=head_patch, cuts=cuts,
                                 want_hidden=want_hidden, want_heads=want_heads)      # a probe that lists nothing is None in it
        args.update(vars(checked))
        bad = [b for b, n in enumerate(plens) if n + max_new_tokens > limit]
        if bad and (overlong == "raise" or len(bad) == len(plens)):
            raise ValueError(f"prompt + new tokens of row(s) {bad} ({[plens[b] + max_new_tokens for b in bad]} positions) "
                             f"exceed max_pos {c.max_pos}")
        eos = c.eos_id if eos_id is None else eos_id            # an id, or HF's list form (one or two ids: binding._eos_pair)
        eos = tuple(int(e) for e in eos) if isinstance(eos, (tuple, list)) else int(eos)
        pad = c.pad_id if pad_id is None else pad_id
        if suppress_eos:
            eos = -1  # benchmark mode: exactly max_new_tokens per row
        assert max_new_tokens >= 1
        knobs = None
        if num_beams != 1:
            if num_beams < 1:
                raise ValueError(f"num_beams must be >= 1, not {num_beams}")
            if do_sample or want_step_logits:
                raise NotImplementedError("beam search runs without sampling (HF's beam-sample mode) and without a per-step logits trace")
            if num_beams > 8 or max_new_tokens > 64:      # the step kernel's state (include/icl_hip.h)
                raise ValueError(f"beam search supports num_beams <= 8 and max_new_tokens <= 64 (got {num_beams}, {max_new_tokens})")
        elif do_sample or repetition_penalty != 1.0:
            # HF's TopKLogitsWarper clamps top_k to the vocabulary; 0 / None switch it off.  The kernel takes 1..SAMPLE_TOP_K_MAX, or
            # the vocabulary size for "off" (full-row normalisation, nucleus over the 1024 most likely tokens); anything else is
            # a caller's argument error, never a device-side failure
            top_k = c.vocab if not top_k else min(int(top_k), c.vocab)
            if top_k < 1 or B.SAMPLE_TOP_K_MAX < top_k < c.vocab:
                raise ValueError(f"top_k={top_k}: the sampling kernel supports 1..{B.SAMPLE_TOP_K_MAX}, or 0 / None / >= vocabulary "
                                 f"({c.vocab}) for no top-k filter")
            if (do_sample and not (0.0 < float(top_p) <= 1.0 and float(temperature) > 0.0)) or not float(repetition_penalty) > 0.0:
                raise ValueError(f"sampling knobs out of range: temperature={temperature} (> 0), top_p={top_p} (0 < p <= 1), "
                                 f"repetition_penalty={repetition_penalty} (> 0)")
            knobs = ((float(temperature), top_k, float(top_p)) if do_sample else (1.0, 1, 1.0)) + (float(repetition_penalty),)
        # ---- 2. drop over-long rows: the same call over the rows that fit
        if bad:
            keep = [b for b in range(len(plens)) if b not in set(bad)]
            if constraint is not None:
                args["constraint"] = (constraint[0], [constraint[1][b] for b in keep])
            args.update(vars(checked.kept(keep)))
            return _undrop(self.generate([prompts[b] for b in keep], speech, **args), keep, bad, len(plens), pad)
        # ---- 3. beams
        if num_beams != 1:
            return self._generate_beam(prompts, speech, max_new_tokens, eos, pad, num_beams, float(length_penalty),
                                       want_first_logits, cache_len_multiple, debug=beam_debug,
                                       repetition_penalty=float(repetition_penalty))
        # ---- 4. prefill
        h, lens = self.embed_prompts(prompts, speech)
        Bn = len(lens)
        max_len = self._cache_len(lens, max_new_tokens, cache_len_multiple)
        cache = self._cache(Bn, max_len)
        marks = getattr(self, "phase_marks", None)     # optional {name: torch.cuda.Event}: bench.py times prefill / decode with it
        if marks is not None:
            marks["prefill_start"].record()
        probes = checked.state(ws, c, Bn, max_len)
        hidden, head_out = probes.capture, probes.head_capture
        logits = self._prefill_logits(h, lens, cache, ws.get("gen_last", (Bn, c.hidden), F32), probes=probes)
        first = logits.clone() if want_first_logits else None
        trace = ws.get("gen_logits_trace", (max_new_tokens, Bn, c.vocab), F32) if want_step_logits else None
        if trace is not None:
            trace[0].copy_(logits)
        if marks is not None:
            marks["prefill_end"].record()
        # ---- 5. the tail of every step, 6. step 0 (on the prefill's logits)
        finished, nxt = ws.get("gen_finished", (Bn,), I32), ws.get("gen_next", (Bn,), I32)
        toks = ws.get("gen_tokens", (Bn, max_new_tokens), I32)
        finished.zero_()
        tail, tail_key, lps = self._decode_tail((finished, toks, nxt), max_new_tokens, eos, pad, constraint, knobs, do_sample,
                                                generator, sample_debug)
        tail(logits, 0)
        # ---- 7. the decode steps
        steps = max_new_tokens - 1
        if steps:
            pos_all, len_all, sid = self._step_tables(lens, steps)
            step_probes = probes.decode_steps()     # None: the decode steps are the plain ones

            def decode_loop():
                for t in range(steps):
                    lg = self.llama.decode_step(ws, cache, nxt, pos_all[t], len_all[t], sid, probes=step_probes)
                    if trace is not None:
                        trace[t + 1].copy_(lg)
                    tail(lg, t + 1)
            self._run_decode((Bn, max_len, steps, eos, pad, tail_key, trace is not None, self.kv_dtype) + probes.graph_key(), decode_loop)
        if marks is not None:
            marks["decode_end"].record()
        # ---- 8. collect: the first host sync of the call, and its only D2H (two with a constraint)
        out = toks.cpu().to(torch.int64)
        width = max_new_tokens
        if B._eos_pair(eos)[0] >= 0:
            is_eos = torch.isin(out, torch.tensor([e for e in B._eos_pair(eos) if e >= 0]))
            first_eos = torch.where(is_eos.any(1), is_eos.float().argmax(1) + 1, torch.full((Bn,), max_new_tokens))
            width = int(first_eos.max())
        res = GenerateResult(tokens=out[:, :width].contiguous(), first_logits=first,
                             step_logits=trace.clone() if trace is not None else None,
                             token_logprobs=lps.cpu()[:, :width].contiguous() if lps is not None else None)
        if hidden is not None:
            res.hidden = hidden.clone()
        if head_out is not None:
            res.head_out = head_out.clone()
        return res

    # ---- the residual stream at the deciding rows: the logit lens and generate(patch=...) ----
    def layer_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        """The logit lens: what every site would answer.  ``hidden`` f32 [B, n_layers + 1, hidden] (``generate(want_hidden=True)``)
        -> f32 [B, n_layers + 1, V] on the device: the final norm and the LM head on every site's row, through
        ``LlamaHIP.logits`` over the B rows of a site — the launches generation makes for its first logits, so site n_layers is
        ``first_logits`` bit for bit."""
        c = self.lm_cfg
        if not (isinstance(hidden, torch.Tensor) and hidden.dtype == F32 and hidden.dim() == 3
                and tuple(hidden.shape[1:]) == (c.n_layers + 1, c.hidden)):
            raise ValueError(f"hidden must be f32 [B, {c.n_layers + 1}, {c.hidden}]")
        hidden = hidden.to(self.device)
        out = torch.empty((hidden.shape[0], c.n_layers + 1, c.vocab), dtype=F32, device=self.device)
        for site in range(c.n_layers + 1):
            out[:, site].copy_(self.llama.logits(self.ws, hidden[:, site].contiguous(), name="lens_logits"))
        return out

    HEAD_CONTRIB_TILE = 2      # the 64x64 tile, whatever the batch: a row's bits do not depend on its neighbours

    def head_contrib(self, head_out: torch.Tensor, heads) -> torch.Tensor:
        """What single heads add to the residual stream.  ``head_out`` bf16 [B, n_layers, n_heads, head_dim]
        (``generate(want_heads=True)``), ``heads`` [(layer, head), ...] -> f32 [B, n_pairs, hidden] on the device: for pair (l, h)
        ``head_out[:, l, h] @ Wo_l[:, h*D:(h+1)*D]^T``, the summand the layer's ``o`` GEMM adds to the stream for that head — one
        icl_gemm_bf16 launch per pair on the column slice of the weight (K = head_dim, lda = the capture's row stride, ldw =
        hidden, f32 output) on ``HEAD_CONTRIB_TILE``.  In FP8 weight mode Wo is W', the bf16 weight the prefill multiplies by."""
        c = self.lm_cfg
        D = c.head_dim
        if not (isinstance(head_out, torch.Tensor) and head_out.dtype == BF16 and head_out.dim() == 4
                and tuple(head_out.shape[1:]) == (c.n_layers, c.n_heads, D)):
            raise ValueError(f"head_out must be bf16 [B, {c.n_layers}, {c.n_heads}, {D}]")
        pairs = P.check_head_pairs(heads, c, "head_contrib")
        head_out = head_out.to(self.device).contiguous()
        out = torch.empty((head_out.shape[0], len(pairs), c.hidden), dtype=F32, device=self.device)
        for i, (l, h) in enumerate(pairs):
            B.gemm(head_out[:, l, h], self.llama.w.layers[l].wo[:, h * D:(h + 1) * D], out[:, i], K=D, tile=self.HEAD_CONTRIB_TILE)
        return out

    # ---- the prompt-attention readout: generate()'s prefill plus one launch per layer ----
    def prompt_attention(self, prompts, speech: Optional[torch.Tensor], segments: Sequence[Sequence[int]],
                         want_probs: bool = False, n_seg: Optional[int] = None, cache_len_multiple: int = 64,
                         want_flow: bool = False) -> PromptAttention:
        """Where the last prompt row (the query that decides the first generated token) looks: its attention mass in every
        layer and head, summed over each segment of the prompt — what ``output_attentions=True`` of a transformers decoder gives
        for that row, reduced per segment (``[B, n_layers, n_heads, n_seg]`` floats; the full last-row weights with
        ``want_probs``).

        ``segments``: one sequence of ints per prompt, as long as the prompt's positions: the segment (0 .. n_seg - 1) of every
        position; an id >= n_seg (``IGNORE_SEGMENT``) is counted nowhere.  ``n_seg`` defaults to 1 + the largest id below
        ``IGNORE_SEGMENT``; at most 32.

        ``want_flow``: also ``flow`` f32 [B, n_layers, n_heads, n_seg, n_seg] and ``rows`` int64 [B, n_seg], both on the CPU — the
        descriptive side of ``generate(cuts=...)``: ``flow[b, l, h, a, c]`` is the attention mass the query rows of segment a
        send to the keys of segment c (causal softmax of every row, summed over the rows; ``rows[b, a]`` of them), one more
        launch per layer (icl_attn_segflow_bf16).  It reads every query of every layer, so the last layer runs at full height
        and its last rows are gathered: the same bits for ``first_logits`` and ``mass``.  An ignored id on a query row: the row is
        summed nowhere.

        Runs the prefill ``generate`` runs (same kernels, same KV cache, last rows only, same chunks), with one more launch per
        layer (icl_attn_segmass_bf16) between the K append and the attention, so ``first_logits`` are ``generate``'s bit for bit.
        ``ValueError`` before any launch: the FP8 KV cache (its prefill attends to unrounded k, the cache does not hold what the
        attention saw), a segment list of the wrong length, ids outside 0..255, more than 32 segments, a prompt over max_pos."""
        c, ws = self.lm_cfg, self.ws
        plens = self._prompt_lengths(prompts)
        segs, n_seg = P.check_readout(segments, n_seg, self.kv_dtype, plens)
        limit = c.max_pos // cache_len_multiple * cache_len_multiple
        bad = [b for b, n in enumerate(plens) if n + 1 > limit]
        if bad:
            raise ValueError(f"prompt of row(s) {bad} ({[plens[b] for b in bad]} positions, + 1 for the cache) exceeds max_pos {c.max_pos}")
        h, lens = self.embed_prompts(prompts, speech)
        max_len = self._cache_len(lens, 1, cache_len_multiple)
        cache = self._cache(len(lens), max_len)
        readout = P.readout_state(ws, c, segs, n_seg, lens, max_len, want_probs, self.device, want_flow=want_flow)
        logits = self._prefill_logits(h, lens, cache, ws.get("gen_last", (len(lens), c.hidden), F32), probes=P.Probes(readout=readout))
        res = PromptAttention(mass=readout.mass.cpu().transpose(0, 1).contiguous(),
                              probs=None if readout.probs is None else readout.probs.transpose(0, 1).clone(),
                              first_logits=logits.clone(), lens=list(lens))
        if readout.flow is not None:
            res.flow = readout.flow.cpu().transpose(0, 1).contiguous()
            res.rows = torch.stack([torch.bincount(sg[sg < n_seg], minlength=n_seg) for sg in segs])
        return res

    def _check_constraint(self, constraint, n_rows: int, max_new_tokens: int, eos_id, do_sample: bool, repetition_penalty: float,
                          num_beams: int, suppress_eos: bool):
        """Host validation of ``generate(constraint=...)``: everything is a ``ValueError`` (a caller's mistake, never a device
        failure) and is raised before any launch.  Returns ``(automaton, [start states as ints])``."""
        try:
            automaton, starts = constraint
            starts = [int(x) for x in starts]
        except (TypeError, ValueError):
            raise ValueError("constraint must be (LabelAutomaton, one start state per prompt)") from None
        c = self.lm_cfg
        if do_sample or float(repetition_penalty) != 1.0 or num_beams != 1 or suppress_eos:
            raise ValueError("constrained decoding is greedy: do_sample, repetition_penalty != 1, num_beams > 1 and suppress_eos "
                             "cannot be combined with a constraint")
        if len(starts) != n_rows:
            raise ValueError(f"{len(starts)} start states for {n_rows} prompts")
        if any(not -1 <= x < automaton.n_states for x in starts):
            raise ValueError(f"start state outside [-1,{automaton.n_states})")
        if automaton.vocab > c.vocab:
            raise ValueError(f"automaton built for a vocabulary of {automaton.vocab} ids, the model has {c.vocab}")
        eos = c.eos_id if eos_id is None else eos_id
        if automaton.eos_id not in B._eos_pair(tuple(eos) if isinstance(eos, (tuple, list)) else eos):
            raise ValueError(f"automaton built for EOS id {automaton.eos_id}, generate() stops on {eos}")
        short = [b for b, x in enumerate(starts) if automaton.min_tokens(x) > max_new_tokens]
        if short:
            raise ValueError(f"max_new_tokens={max_new_tokens} is below the shortest answer of row(s) {short[:8]} "
                             f"({[automaton.min_tokens(starts[b]) for b in short[:8]]} tokens): no complete label fits")
        return automaton, starts

    def _generate_beam(self, prompts, speech, max_new_tokens: int, eos: int, pad: int, K: int, length_penalty: float,
                       want_first_logits: bool, cache_len_multiple: int, debug: Optional[dict] = None,
                       repetition_penalty: float = 1.0) -> GenerateResult:
        """HF beam search with ``inputs_embeds`` only (models/custom_salmon.py:704-715; transformers `_beam_search`,
        early_stopping=False).  The prompt is prefilled ONCE per row (HF prefills K copies), its K/V rows are copied to the
        row's K beams, and every step is `icl_beam_step` (log-softmax, the 2K best continuations, running / finished
        bookkeeping) -> copy of the generated K/V positions from each beam's parent (`icl_kv_copy_spans_bf16`: the prompt part
        is identical across a row's beams, so HF's whole-cache reorder is a copy of <= max_new_tokens positions) -> one
        decode step over rows x K sequences.  Nothing synchronises with the host until the final D2H of the best hypotheses;
        rows whose search has ended keep stepping with their finished slots frozen (HF stops its loop instead: same result).
        ``debug`` (tests; single pass only): receives per step the logits the step scored, and the running sequences / parents /
        tokens it chose."""
        c, ws = self.lm_cfg, self.ws
        n_rows = len(prompts)
        per_pass = max(1, self.beam_rows // K)
        if n_rows > per_pass:                                  # rows x beams beyond the decode tile: run the rows in groups
            assert debug is None
            parts = [self._generate_beam(prompts[i:i + per_pass], speech, max_new_tokens, eos, pad, K, length_penalty,
                                         want_first_logits, cache_len_multiple, repetition_penalty=repetition_penalty)
                     for i in range(0, n_rows, per_pass)]
            width = max(p.tokens.shape[1] for p in parts)
            toks = torch.full((n_rows, width), pad, dtype=torch.int64)
            r = 0
            for p in parts:
                toks[r:r + p.tokens.shape[0], :p.tokens.shape[1]] = p.tokens
                r += p.tokens.shape[0]
            first = torch.cat([p.first_logits for p in parts]) if want_first_logits else None
            return GenerateResult(tokens=toks, first_logits=first)
        h, lens = self.embed_prompts(prompts, speech)
        Bn, T = len(lens), max_new_tokens
        BK = Bn * K
        # the beams' sequences first, then the rows the prompts prefill into
        whole = self._cache(BK + Bn, self._cache_len(lens, T, cache_len_multiple))
        cache, pre = whole.rows(0, BK), whole.rows(BK, BK + Bn)
        logits = self._prefill_logits(h, lens, pre, ws.get("gen_last", (Bn, c.hidden), F32))
        first = logits.clone() if want_first_logits else None
        st = B.BeamState(ws.get, Bn, K, T, pad)

        def score(lg, step):
            B.beam_step(lg, st, step, eos, length_penalty, V=c.vocab, repetition_penalty=repetition_penalty)
            if debug is not None:
                for key, val in (("logits", lg), ("run_seq", st.run_seq), ("parent", st.parent), ("next", st.next_ids),
                                 ("fin_seq", st.fin_seq), ("fin_score", st.fin_score), ("fin_len", st.fin_len)):
                    debug.setdefault(key, []).append(val.clone())
        score(logits, 0)
        lens_rep = [s for s in lens for _ in range(K)]
        plen = ws.get("gen_beam_plen", (BK,), I32)
        plen.copy_(torch.tensor(lens_rep, dtype=I32), non_blocking=True)
        if T > 1:
            src = ws.get("gen_beam_src", (BK,), I32)           # beam b*K+k starts from the prompt rows of sequence BK + b
            src.copy_(torch.tensor([BK + b for b in range(Bn) for _ in range(K)], dtype=I32), non_blocking=True)
            for kv, sc in whole.planes():
                B.kv_copy_spans(kv, kv, BK, src_seq=src, n_t=plen, src_scale=sc, dst_scale=sc)
            steps = T - 1
            pos_all, len_all, sid = self._step_tables(lens_rep, steps)
            tmp_k = ws.get("beam_tmp_k", (c.n_layers, BK, c.kv_heads, steps, c.head_dim), cache.k.dtype)
            tmp_v = ws.get("beam_tmp_v", tuple(tmp_k.shape), cache.k.dtype)
            tmp_ks = tmp_vs = None
            if cache.dtype == "fp8":                           # FP8 KV cache: the row scales travel with the row bytes
                tmp_ks = ws.get("beam_tmp_ks", tuple(tmp_k.shape[:4]), F32)
                tmp_vs = ws.get("beam_tmp_vs", tuple(tmp_k.shape[:4]), F32)
            for t in range(steps):
                if t:                                          # the t positions generated so far follow their beam's parent
                    for (kv, sc), tmp, tsc in zip(cache.planes(), (tmp_k, tmp_v), (tmp_ks, tmp_vs)):
                        B.kv_copy_spans(kv, tmp, BK, src_seq=st.parent, src_t0=plen, n_fixed=t, src_scale=sc, dst_scale=tsc)
                        B.kv_copy_spans(tmp, kv, BK, dst_t0=plen, n_fixed=t, src_scale=tsc, dst_scale=sc)
                lg = self.llama.decode_step(ws, cache, st.next_ids, pos_all[t], len_all[t], sid)
                score(lg, t + 1)
        best = st.fin_seq[:, 0].cpu().to(torch.int64)                                   # the only D2H pair of the call
        blen = st.fin_len[:, 0].cpu()
        # 2 x layers x rows x heads x (T-1) x head_dim cache elements (+ the fp8 cache's row scales): not kept between calls
        ws.release("beam_tmp_k", "beam_tmp_v", "beam_tmp_ks", "beam_tmp_vs")
        width = max(1, int(blen.max()))
        return GenerateResult(tokens=best[:, :width].contiguous(), first_logits=first)


class SalmonnRuntime(CausalLMRuntimeMixin):
    def __init__(self, cfg: SalmonnCfg, state_dict: Dict[str, torch.Tensor], device="cuda", consume: bool = False,
                 parts: Sequence[str] = ("whisper", "beats", "qformer", "llama"), llm_weight_dtype: str = "bf16",
                 llm_kv_dtype: str = "bf16"):
        if not torch.cuda.is_available():
            raise B.IclError("SalmonnRuntime needs a GPU: the HIP path has no CPU fallback")
        B.load_library()
        self.cfg = cfg
        self.lm_cfg = cfg.llama
        self.device = torch.device(device)
        self.kv_dtype = check_kv_dtype(llm_kv_dtype, cfg.llama)     # "fp8" + grouped-query attention: ValueError, before any launch
        sd = normalize_keys(state_dict) if not consume else state_dict
        self.ws = Workspace(self.device)
        self.whisper = self.beats = self.qformer = self.llama = None
        if "whisper" in parts:
            self.logmel = LogMel(cfg.whisper.n_mels, self.device)
            self.whisper = WhisperEncoderHIP(pack_whisper(sd, cfg.whisper, self.device, consume=consume))
        if "beats" in parts and cfg.beats is not None:
            self.beats = BeatsHIP(pack_beats(sd, cfg.beats, self.device, consume=consume), self.device)
        if "qformer" in parts:
            self.qformer = SpeechQFormerHIP(pack_qformer(sd, cfg.qformer, self.device, consume=consume),
                                            cfg.whisper.d_model, cfg.beats.d_model if self.beats is not None else 0,
                                            cfg.llama.hidden)
        if "llama" in parts:
            self.llama = LlamaHIP(pack_llama(sd, cfg.llama, self.device, consume=consume), self.device,
                                  weight_dtype=llm_weight_dtype)
        self._graph_reset()

    # --------------------------------------------------------------------------------------------
    # K1-K8: SALMONN.encode_speech
    # --------------------------------------------------------------------------------------------
    @property
    def tokens_per_audio(self) -> int:
        return self.qformer.n_windows(1500)

    def encode_speech(self, raw_wav: Optional[torch.Tensor], wav_lens: Optional[Sequence[int]] = None,
                      spectrogram: Optional[torch.Tensor] = None, padded_lens: Optional[Sequence[int]] = None) -> torch.Tensor:
        """raw_wav f32 [n, L] (zero padded; host or device), wav_lens valid samples per audio.
        spectrogram (optional, f32 [n, n_mels, 3000]): use the caller's log-mel instead of K1.
        padded_lens: length the reference's BEATs would see per audio (defaults to wav_lens: batch-1 semantics).
        Returns speech embeddings f32 [n, 88, H_llm] on the device (atts are all ones in the reference); with a clip longer than
        30 s in the batch: [n, W_max, H_llm] and ``last_audio_windows`` = tokens per audio."""
        ws, dev = self.ws, self.device
        if raw_wav is not None:
            raw_wav = raw_wav.to(device=dev, dtype=F32)
            if raw_wav.dim() == 1:
                raw_wav = raw_wav[None]
            raw_wav = raw_wav.contiguous()
            n = raw_wav.shape[0]
            if wav_lens is None:
                wav_lens = [raw_wav.shape[1]] * n
            wav_lens = [int(x) for x in wav_lens]
        else:
            n = spectrogram.shape[0]
        if spectrogram is not None:
            xt = self.logmel.from_spectrogram(ws, spectrogram.to(device=dev, dtype=F32))
        else:
            xt, _ = self.logmel(ws, raw_wav, _i32(wav_lens, dev))
        speech = self.whisper.forward(ws, xt)
        audio = cu = None
        if self.beats is not None and raw_wav is not None:
            padded = [int(x) for x in (padded_lens if padded_lens is not None else wav_lens)]
            audio, cu, _ = self.beats.forward(ws, raw_wav, padded, wav_lens)
        out = self.qformer.forward(ws, speech, n, audio, cu)
        # tokens per audio: 88 up to 30 s; a longer clip keeps its extra BEATs frames (SALMONN pads the shorter stream) and gets
        # more windows — rows past last_audio_windows[a] of audio a are zero padding, not tokens
        self.last_audio_windows = list(self.qformer.last_windows)
        return out.view(n, max(self.last_audio_windows), self.cfg.llama.hidden)

    def log_mel(self, raw_wav: torch.Tensor, wav_lens: Sequence[int]) -> torch.Tensor:
        """K1 alone: f32 [n, n_mels, 3000] (the ``spectrogram`` batch key of the reference's processor)."""
        raw_wav = raw_wav.to(device=self.device, dtype=F32).contiguous()
        _, spec = self.logmel(self.ws, raw_wav, _i32([int(x) for x in wav_lens], self.device), want_spec=True)
        return spec

