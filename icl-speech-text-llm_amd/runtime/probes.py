"""Probes of the deciding rows of the LLM decoder — the last prompt row of every sequence and the rows generated after it:

  the prompt-attention readout   ``AttnReadout``          icl_attn_segmass_bf16         where the row looks, per prompt segment
  attention knockout             ``Knockout``             icl_attn_decode_masked_bf16   the row attends as if segments were absent
  residual capture / patching    a tensor, ``ResidPatch`` icl_resid_rows_f32            the row's residual stream, read and written
  head-output capture / patching a tensor, ``HeadPatch``  icl_head_rows_bf16            what single heads hand to o_proj, read and written

and of ANY prompt row: attention cuts between prompt segments, ``Cuts`` (icl_attn_cut_rows_bf16; in the decode steps the knockout's
icl_attn_decode_masked_bf16) — a query of one segment attends as if the keys of another were absent.

Host validation (``check_*``), device state (``*_state``), re-slicing to a prefill chunk and to the kept rows of a drop, and
``Probes``, the one bundle handed between runtime/salmonn.py and runtime/engines.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import binding as B
from .engines import F32, I32, Workspace, _i32

MAX_READOUT_SEGMENTS = 32      # icl_attn_segmass_bf16: one thread per (head of a K/V group, segment)
MAX_KNOCKOUT_SEGMENTS = 32     # icl_attn_decode_masked_bf16: one bit of a u32 per segment; ids >= 32 are never blocked
MAX_CUT_SEGMENTS = 32          # icl_attn_cut_rows_bf16: the same bit set per listed row
CUT_KEYS = ("segments", "pairs", "layers", "heads", "generated")
IGNORE_SEGMENT = 255           # a segment id that is counted nowhere and never blocked, whatever n_seg is
PATCH_KEYS = ("site", "vectors", "mode", "alpha", "rows", "steps")
HEAD_PATCH_KEYS = ("heads", "vectors", "mode", "alpha", "rows", "steps")


# ================================================================================================
# Device state: what a launch reads, and the launch
# ================================================================================================
def _listed_rows(listed: Tuple[int, ...], row_seq: torch.Tensor, b0: int, b1: int):
    """Of the ascending sequences ``listed`` (``row_seq``: the same on the device), those of the chunk b0 .. b1-1: None when
    there is none, else (first entry, end entry, the sequences relative to b0, the same on the device)."""
    lo = sum(1 for s in listed if s < b0)
    hi = sum(1 for s in listed if s < b1)
    if lo == hi:
        return None
    if b0 == 0 and hi == len(listed):
        return lo, hi, listed, row_seq
    sub = tuple(s - b0 for s in listed[lo:hi])
    return lo, hi, sub, _i32(sub, row_seq.device)


@dataclass
class AttnReadout:
    """Where a prefill leaves the prompt-attention readout of its sequences, all on the device: ``seg`` uint8 [n_seqs, >= cache
    max_len] the segment of every prompt position (>= n_seg: counted nowhere), ``lens`` int32 [n_seqs] the prompt lengths,
    ``mass`` f32 [n_layers, n_seqs, n_heads, n_seg] and ``probs`` None or f32 [n_layers, n_seqs, n_heads, >= max_len] (written)."""
    seg: torch.Tensor
    lens: torch.Tensor
    mass: torch.Tensor
    probs: Optional[torch.Tensor] = None

    def rows(self, b0: int, b1: int) -> "AttnReadout":
        """The readout of sequences b0 .. b1-1 (views), for a prefill over that chunk of the batch (``KVCache.rows``)."""
        return AttnReadout(self.seg[b0:b1], self.lens[b0:b1], self.mass[:, b0:b1],
                           None if self.probs is None else self.probs[:, b0:b1])

    def launch(self, layer: int, q: torch.Tensor, q_rows: Optional[torch.Tensor], kc: torch.Tensor, cfg, max_len: int) -> None:
        B.attn_segmass(q, kc, self.lens, self.seg, self.mass[layer], cfg.n_heads, cfg.head_dim, max_len, cfg.head_dim ** -0.5,
                       n_kv_heads=cfg.kv_heads, q_rows=q_rows, probs=None if self.probs is None else self.probs[layer])


@dataclass
class Knockout:
    """Attention knockout, all on the device: in decoder layers ``layers[0] .. layers[1] - 1`` the LAST prompt row and every
    generated row of the listed sequences attend as if the keys of their blocked segments were not there
    (icl_attn_decode_masked_bf16 rewrites those rows of the attention output after the layer's ordinary attention launch).
    ``seg`` uint8 [n_seqs, >= cache max_len]: the segment of every cache position, 255 past the prompt (generated positions are
    always visible); ``blocked`` int32 [n_listed, n_heads]: bit g of a (listed row, query head) = segment g is not read;
    ``row_seq`` int32 [n_listed]: the listed sequences, ascending (``listed``: the same on the host).  The runtime keeps all
    three in graph-visible workspace buffers and refills them on every call, so ``uid`` — what a captured decode graph bakes in
    besides those pointers: the number of listed rows (a grid size) and the layer window — keys the decode graphs."""
    seg: torch.Tensor
    blocked: torch.Tensor
    row_seq: torch.Tensor
    listed: Tuple[int, ...]
    layers: Tuple[int, int]

    @property
    def uid(self):
        return ("knockout", len(self.listed), self.layers[0], self.layers[1])

    def rows(self, b0: int, b1: int) -> Optional["Knockout"]:
        """The knockout of sequences b0 .. b1-1 (views; sequence ids relative to b0), for a prefill over that chunk of the
        batch (``KVCache.rows``); None when the chunk lists no row."""
        part = _listed_rows(self.listed, self.row_seq, b0, b1)
        if part is None:
            return None
        lo, hi, sub, row_seq = part
        return Knockout(self.seg[b0:b1], self.blocked[lo:hi], row_seq, sub, self.layers)

    def covers(self, layer: int) -> bool:
        return self.layers[0] <= layer < self.layers[1]

    def launch(self, q: torch.Tensor, att: torch.Tensor, row_q: torch.Tensor, kc, vc, lens: torch.Tensor, cfg, max_len: int) -> None:
        """Rewrite rows ``row_q`` (int32 [n_listed]) of ``att`` from the same rows of ``q`` (rotated) over the bf16 cache."""
        B.attn_decode_masked(q, kc, vc, att, lens, self.seg, self.blocked, self.row_seq, row_q, cfg.n_heads, cfg.head_dim, max_len,
                             cfg.head_dim ** -0.5, n_kv_heads=cfg.kv_heads)


@dataclass
class ResidPatch:
    """Residual-stream patching at the deciding rows, all on the device: at site ``site`` (0 .. n_layers - 1: the input of that
    decoder layer, before its norm; n_layers: the output of the last layer, before the final norm) the LAST prompt row of the
    listed sequences — and with ``steps == "all"`` every generated row — is replaced by its vector, or gets ``alpha`` times its
    vector added (icl_resid_rows_f32).  ``vectors`` f32 [n_listed, hidden], or [1, hidden]: one vector for all listed rows;
    ``row_seq`` int32 [n_listed]: the listed sequences, ascending and distinct (``listed``: the same on the host).  The runtime
    keeps both tensors in graph-visible workspace buffers and refills them on every call, so ``uid`` — what a captured decode
    graph bakes in besides those pointers: the number of listed rows (a grid size), whether the vector is shared (a leading
    dimension), site, mode, steps and alpha, a by-value kernel argument — keys the decode graphs."""
    vectors: torch.Tensor
    row_seq: torch.Tensor
    listed: Tuple[int, ...]
    site: int
    mode: str = "replace"
    alpha: float = 1.0
    steps: str = "prompt"

    @property
    def uid(self):
        return ("resid_patch", len(self.listed), int(self.vectors.shape[0]), self.site, self.mode, self.steps, float(self.alpha))

    def rows(self, b0: int, b1: int) -> Optional["ResidPatch"]:
        """The patch of sequences b0 .. b1-1 (views; sequence ids relative to b0), for a prefill over that chunk of the batch
        (``KVCache.rows``); None when the chunk lists no row."""
        part = _listed_rows(self.listed, self.row_seq, b0, b1)
        if part is None:
            return None
        lo, hi, sub, row_seq = part
        return replace(self, vectors=self.vectors if self.vectors.shape[0] == 1 else self.vectors[lo:hi], row_seq=row_seq, listed=sub)

    def launch(self, h: torch.Tensor, rows: torch.Tensor, capture: Optional[torch.Tensor] = None) -> None:
        """Patch rows ``rows`` (int32 [n_listed]) of ``h``; ``capture`` f32 [n_listed, hidden] receives their pre-patch bits."""
        B.resid_rows(h, rows, capture=capture, vec=self.vectors, mode=self.mode, alpha=self.alpha)


@dataclass
class HeadPatch:
    """Attention-head output patching at the deciding rows, all on the device: in the attention output of a decoder layer — the
    operand of its o_proj — the selected heads of the LAST prompt row of the listed sequences, and with ``steps == "all"`` of
    every generated row, are replaced by their vectors, or get ``alpha`` times their vectors added (icl_head_rows_bf16).
    ``heads`` int32 [n_pairs]: the head indices of the (layer, head) pairs, sorted by layer and head; ``layers``: (layer, first
    pair, end pair) of every layer with a selected head, ascending; ``vectors`` f32 [n_listed, n_pairs, head_dim] in that order
    of pairs, or [1, n_pairs, head_dim]: one block for all listed rows; ``row_seq`` int32 [n_listed]: the listed sequences,
    ascending and distinct (``listed``: the same on the host).  The runtime keeps the three tensors in graph-visible workspace
    buffers and refills them on every call, so ``uid`` — what a captured decode graph bakes in besides those pointers: the number
    of listed rows (a grid size), whether the vectors are shared (a leading dimension), the layers that launch with their head
    counts (grid sizes and offsets into the buffers), mode, steps and alpha, a by-value kernel argument — keys the decode graphs."""
    vectors: torch.Tensor
    heads: torch.Tensor
    row_seq: torch.Tensor
    listed: Tuple[int, ...]
    layers: Tuple[Tuple[int, int, int], ...]
    mode: str = "replace"
    alpha: float = 1.0
    steps: str = "prompt"

    @property
    def uid(self):
        return ("head_patch", len(self.listed), int(self.vectors.shape[0]), tuple((l, p1 - p0) for l, p0, p1 in self.layers), self.mode,
                self.steps, float(self.alpha))

    def rows(self, b0: int, b1: int) -> Optional["HeadPatch"]:
        """The patch of sequences b0 .. b1-1 (views; sequence ids relative to b0), for a prefill over that chunk of the batch
        (``KVCache.rows``); None when the chunk lists no row."""
        part = _listed_rows(self.listed, self.row_seq, b0, b1)
        if part is None:
            return None
        lo, hi, sub, row_seq = part
        return replace(self, vectors=self.vectors if self.vectors.shape[0] == 1 else self.vectors[lo:hi], row_seq=row_seq, listed=sub)

    def pairs(self, layer: int) -> Optional[Tuple[int, int]]:
        """(first pair, end pair) of ``layer``, or None: no head of the layer is selected."""
        return next(((p0, p1) for l, p0, p1 in self.layers if l == layer), None)

    def launch(self, layer: int, att: torch.Tensor, rows: torch.Tensor, cfg, capture: Optional[torch.Tensor] = None) -> None:
        """Patch the layer's selected heads in rows ``rows`` (int32 [n_listed]) of ``att``; ``capture`` bf16 [n_listed, n_heads *
        head_dim] receives the rows' pre-patch bits."""
        p0, p1 = self.pairs(layer)
        B.head_rows(att, rows, n_heads=cfg.n_heads, head_dim=cfg.head_dim, capture=capture, heads=self.heads[p0:p1],
                    vec=self.vectors[:, p0:p1], mode=self.mode, alpha=self.alpha)


@dataclass
class Cuts:
    """Attention cuts between prompt segments: in decoder layers ``layers[0] .. layers[1] - 1`` and the query heads that are on, a
    query of segment s at ANY prompt position attends as if the keys of the segments K(s) cut for it were absent
    (icl_attn_cut_rows_bf16 rewrites the listed rows of the attention output after the layer's ordinary attention launch).
    ``entries[b]``: the listed positions of sequence b, ascending, and their u32 bit sets, two int64 arrays ``(positions, masks)``
    — on the HOST: a prefill builds its tile tables from them (``tile_tables``), ``tile_rows`` rows of one sequence per tile.  ``seg`` uint8
    [n_seqs, >= cache max_len]: the segment of every cache position, 255 past the prompt (generated positions are always
    visible); ``head_on``: None (all heads) or uint8 [n_heads].  The decode steps' state, for the sequences whose generated rows
    cut something (``gen_listed``, ascending; ``gen_row_seq``: the same on the device): ``gen_blocked`` int32 [n_listed,
    n_heads], the knockout's operand of icl_attn_decode_masked_bf16.  ``seg``, ``head_on`` and the decode state live in
    graph-visible workspace buffers refilled on every call, so ``uid`` — what a captured decode graph bakes in besides those
    pointers: the number of sequences listed in the decode steps (a grid size) and the layer window — keys the decode graphs;
    nothing of the prefill's tables reaches a decode graph."""
    seg: torch.Tensor
    entries: Tuple[Tuple[np.ndarray, np.ndarray], ...]
    layers: Tuple[int, int]
    n_layers: int
    tile_rows: int
    head_on: Optional[torch.Tensor] = None
    gen_listed: Tuple[int, ...] = ()
    gen_row_seq: Optional[torch.Tensor] = None
    gen_blocked: Optional[torch.Tensor] = None

    @property
    def uid(self):
        return ("cuts", len(self.gen_listed), self.layers[0], self.layers[1])

    def rows(self, b0: int, b1: int) -> Optional["Cuts"]:
        """The cuts of sequences b0 .. b1-1 (views; sequence ids relative to b0), for a prefill over that chunk of the batch
        (``KVCache.rows``); None when the chunk lists no row.  The decode state stays behind: a prefill does not read it."""
        if not any(len(pos) for pos, _ in self.entries[b0:b1]):
            return None
        return Cuts(self.seg[b0:b1], self.entries[b0:b1], self.layers, self.n_layers, self.tile_rows, self.head_on)

    def covers(self, layer: int) -> bool:
        return self.layers[0] <= layer < self.layers[1]

    def tile_tables(self, seq_lens: List[int], cu_h: Optional[List[int]], last_only: bool, device, max_tiles: int = 65535):
        """The tile tables of a prefill, one tuple (tile_seq, row_q, row_len, blocked) of int32 device tensors per launch (a
        launch holds at most ``max_tiles`` tiles).  Entries ascend by (sequence, position) and a tile holds ``tile_rows``
        consecutive entries of ONE sequence, so its row_lens are close; the tail of a sequence's last tile is empty slots (row_q
        -1).  Position p of sequence b is row ``cu_h[b] + p`` of Q / O, or with ``cu_h`` None (gathered last rows) row b.
        ``last_only``: only the sequences' last positions (the model's last layer, where no other row can influence anything)."""
        R = self.tile_rows
        tile_seq, row_q, row_len, blocked = [], [], [], []
        for b, (pos, msk) in enumerate(self.entries):
            if last_only:
                keep = pos == seq_lens[b] - 1
                pos, msk = pos[keep], msk[keep]
            if not len(pos):
                continue
            n_tiles = -(-len(pos) // R)
            pad = np.zeros(n_tiles * R - len(pos), dtype=np.int64)
            tile_seq.append(np.full(n_tiles, b, dtype=np.int64))
            row_q.append(np.concatenate([pos + cu_h[b] if cu_h is not None else np.full(len(pos), b, dtype=np.int64), pad - 1]))
            row_len.append(np.concatenate([pos + 1, pad]))
            blocked.append(np.concatenate([np.where(msk >= 1 << 31, msk - (1 << 32), msk), pad]))     # the u32 bit set in an int32
        if not tile_seq:
            return []
        tile_seq, row_q, row_len, blocked = (np.concatenate(x) for x in (tile_seq, row_q, row_len, blocked))
        tile_seq, row_q, row_len, blocked = (x.astype(np.int32) for x in (tile_seq, row_q, row_len, blocked))
        return [(_i32(tile_seq[i:i + max_tiles], device),) + tuple(_i32(x[i * R:(i + max_tiles) * R], device) for x in (row_q, row_len, blocked))
                for i in range(0, len(tile_seq), max_tiles)]

    def launch(self, tables, q: torch.Tensor, att: torch.Tensor, kc, vc, cfg, max_len: int) -> None:
        """Rewrite the rows of ``att`` that ``tables`` list from the same rows of ``q`` (rotated) over the bf16 cache."""
        for tile_seq, row_q, row_len, blocked in tables:
            B.attn_cut_rows(q, kc, vc, att, self.seg, tile_seq, row_q, row_len, blocked, cfg.n_heads, cfg.head_dim, max_len,
                            cfg.head_dim ** -0.5, tile_rows=self.tile_rows, n_kv_heads=cfg.kv_heads, head_on=self.head_on)

    def launch_step(self, q: torch.Tensor, att: torch.Tensor, kc, vc, lens: torch.Tensor, cfg, max_len: int) -> None:
        """A decode step: the generated rows of the listed sequences under K(generated), the knockout's launch."""
        B.attn_decode_masked(q, kc, vc, att, lens, self.seg, self.gen_blocked, self.gen_row_seq, self.gen_row_seq, cfg.n_heads,
                             cfg.head_dim, max_len, cfg.head_dim ** -0.5, n_kv_heads=cfg.kv_heads)


# ================================================================================================
# The bundle the layers hand to each other
# ================================================================================================
@dataclass
class Probes:
    """The probes of one call, each optional: what ``generate`` / ``prompt_attention`` build, ``_prefill_logits`` slices per
    chunk and ``LlamaHIP.prefill`` / ``_last_layer_rows`` / ``decode_step`` call at their hook points.  ``capture``: f32 [n_seqs,
    n_layers + 1, hidden], receives the residual stream of every sequence's last prompt row at every site, pre-patch;
    ``head_capture``: bf16 [n_seqs, n_layers, n_heads, head_dim], receives the head outputs of that row in every layer, as o_proj
    would have read them (after a knockout's rewrite), before a head patch."""
    readout: Optional[AttnReadout] = None
    knockout: Optional[Knockout] = None
    capture: Optional[torch.Tensor] = None
    patch: Optional[ResidPatch] = None
    head_capture: Optional[torch.Tensor] = None
    head_patch: Optional[HeadPatch] = None
    cuts: Optional[Cuts] = None
    # host tables of the prefill in progress (``start_prefill``), all int32 on the device: the sequences' last packed rows, the
    # prompt lengths as the masked launch's key counts, the last packed rows of the knockout's, of the patch's and of the head
    # patch's listed sequences
    _last: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    _key_counts: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    _ko_last: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    _pt_last: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    _hp_last: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    # ... and what the cuts' tile tables are built from and kept in: (prompt lengths, first packed rows), tables by (last rows
    # only, packed rows)
    _ct_prefill: Optional[tuple] = field(default=None, init=False, repr=False)
    _ct_tables: dict = field(default_factory=dict, init=False, repr=False)

    def _or_none(self) -> Optional["Probes"]:
        return None if all(p is None for p in (self.readout, self.knockout, self.capture, self.patch, self.head_capture,
                                               self.head_patch, self.cuts)) else self

    def rows(self, b0: int, b1: int) -> Optional["Probes"]:
        """The bundle of a prefill over sequences b0 .. b1-1.  A probe that lists no row of the chunk is absent from it, and a
        bundle with nothing left is None: the chunk then launches what it launches without probes."""
        return Probes(None if self.readout is None else self.readout.rows(b0, b1),
                      None if self.knockout is None else self.knockout.rows(b0, b1),
                      None if self.capture is None else self.capture[b0:b1],
                      None if self.patch is None else self.patch.rows(b0, b1),
                      None if self.head_capture is None else self.head_capture[b0:b1],
                      None if self.head_patch is None else self.head_patch.rows(b0, b1),
                      None if self.cuts is None else self.cuts.rows(b0, b1))._or_none()

    def decode_steps(self) -> Optional["Probes"]:
        """The bundle of the decode steps: the knockout, a patch and a head patch of every step, and cuts whose generated rows
        cut something; None when the steps are the plain ones."""
        return Probes(knockout=self.knockout, patch=self.patch if self.patch is not None and self.patch.steps == "all" else None,
                      head_patch=self.head_patch if self.head_patch is not None and self.head_patch.steps == "all" else None,
                      cuts=self.cuts if self.cuts is not None and self.cuts.gen_listed else None)._or_none()

    def graph_key(self) -> tuple:
        """What a captured decode loop bakes in of its probes besides pointers: appended to the graph key of the plain call."""
        every_step = (self.knockout, self.patch if self.patch is not None and self.patch.steps == "all" else None,
                      self.head_patch if self.head_patch is not None and self.head_patch.steps == "all" else None,
                      self.cuts if self.cuts is not None and self.cuts.gen_listed else None)
        return tuple(p.uid for p in every_step if p is not None)

    # ---- a prefill: preconditions and host tables, once per call of LlamaHIP.prefill ----
    def start_prefill(self, seq_lens: List[int], cu_h: List[int], last_idx: Optional[torch.Tensor], cache) -> None:
        """``last_idx``: int32 [n_seqs], the sequences' last packed rows, or None without ``last_rows_only``."""
        last, bf16 = last_idx is not None, cache is not None and cache.dtype == "bf16"
        assert self.readout is None or (last and bf16), "the attention readout reads the last rows' q and a bf16 K cache"
        assert self.knockout is None or (last and bf16), "attention knockout rewrites the last rows from a bf16 KV cache"
        assert (self.capture is None and self.patch is None) or last, "residual capture / patching works on the last rows (last_rows_only)"
        assert (self.head_capture is None and self.head_patch is None) or last, "head capture / patching works on the last rows (last_rows_only)"
        assert self.cuts is None or (last and bf16), "attention cuts rewrite the listed rows from a bf16 KV cache (last_rows_only)"
        self._ct_prefill, self._ct_tables = (list(seq_lens), list(cu_h)), {}
        ko, pt, hp = self.knockout, self.patch, self.head_patch
        self._last = last_idx
        self._key_counts = None if ko is None else _i32(seq_lens, last_idx.device)
        self._ko_last = None if ko is None else _i32([cu_h[b + 1] - 1 for b in ko.listed], last_idx.device)
        self._pt_last = None if pt is None else _i32([cu_h[b + 1] - 1 for b in pt.listed], last_idx.device)
        self._hp_last = None if hp is None else _i32([cu_h[b + 1] - 1 for b in hp.listed], last_idx.device)

    # ---- the three hook points of a layer.  ``packed``: the rows of h / q / att are the packed rows of a prefill, where the
    # deciding row of a sequence is its last one; otherwise row b is sequence b's (a decode step, the gathered last rows) ----
    def residual_site(self, site: int, h: torch.Tensor, packed: bool = False) -> bool:
        """Site ``site`` of the residual stream ``h`` (the top of layer ``site``; n_layers: after the last layer):
        ``capture[:, site]`` receives the deciding row of every sequence, and a patch at this site rewrites those of its listed
        sequences.  One launch does both when the patch lists every sequence; a patch of some sequences next to a capture of all
        is a capture launch and then a patch launch.  True when rows of ``h`` were rewritten."""
        cap = None if self.capture is None else self.capture[:, site]
        pt = self.patch if self.patch is not None and self.patch.site == site else None
        if cap is not None:
            n = cap.shape[0]
            all_rows = self._last if packed else _i32(list(range(n)), h.device)
            if pt is not None and pt.listed == tuple(range(n)):
                pt.launch(h, all_rows, capture=cap)
                return True
            B.resid_rows(h, all_rows, capture=cap)
        if pt is not None:
            pt.launch(h, self._pt_last if packed else pt.row_seq)
        return pt is not None

    def keys_appended(self, layer: int, q: torch.Tensor, kc: torch.Tensor, cfg, max_len: int, packed: bool = False) -> None:
        """q is rotated and the layer's k is in the bf16 cache ``kc``: the readout of the deciding rows' attention."""
        if self.readout is not None:
            self.readout.launch(layer, q, self._last if packed else None, kc, cfg, max_len)

    def attention_written(self, layer: int, q: torch.Tensor, att: torch.Tensor, kc, vc, cfg, max_len: int,
                          lens: Optional[torch.Tensor] = None, packed: bool = False) -> None:
        """The layer's attention output is in ``att``: a knockout that covers the layer rewrites the listed deciding rows under
        their masks.  ``lens``: int32 [n_seqs] key counts (a decode step's; None in a prefill: the prompt lengths).  Then the
        head outputs, as o_proj is about to read them: ``head_capture[:, layer]`` receives the deciding row of every sequence, and
        a head patch with a selected head in this layer rewrites those heads in the rows of its listed sequences.  One launch
        does both when the patch lists every sequence; a patch of some sequences next to a capture of all is a capture launch
        and then a patch launch (``residual_site``'s rule).  A layer with neither launches nothing."""
        ko, ct = self.knockout, self.cuts
        if ko is not None and ko.covers(layer):
            ko.launch(q, att, self._ko_last if packed else ko.row_seq, kc, vc, self._key_counts if lens is None else lens, cfg, max_len)
        if ct is not None and ct.covers(layer):
            if lens is not None:
                ct.launch_step(q, att, kc, vc, lens, cfg, max_len)
            else:
                ct.launch(self._cut_tables(layer == ct.n_layers - 1, packed, att.device), q, att, kc, vc, cfg, max_len)
        cap = None if self.head_capture is None else self.head_capture[:, layer].flatten(1)
        hp = self.head_patch if self.head_patch is not None and self.head_patch.pairs(layer) is not None else None
        if cap is not None:
            n = cap.shape[0]
            all_rows = self._last if packed else _i32(list(range(n)), att.device)
            if hp is not None and hp.listed == tuple(range(n)):
                return hp.launch(layer, att, all_rows, cfg, capture=cap)
            B.head_rows(att, all_rows, n_heads=cfg.n_heads, head_dim=cfg.head_dim, capture=cap)
        if hp is not None:
            hp.launch(layer, att, self._hp_last if packed else hp.row_seq, cfg)

    def _cut_tables(self, last_only: bool, packed: bool, device):
        """The cuts' tile tables of the prefill in progress, built once per (last rows only, packed rows).  In the model's last
        layer only the sequences' last rows can influence anything, so only they are launched — exact, not an approximation;
        where that layer is trimmed (``packed`` False) row b of q / att is sequence b's last row."""
        key = (last_only, packed)
        if key not in self._ct_tables:
            seq_lens, cu_h = self._ct_prefill
            assert packed or last_only, "gathered rows hold the sequences' last rows only"
            self._ct_tables[key] = self.cuts.tile_tables(seq_lens, cu_h if packed else None, last_only, device)
        return self._ct_tables[key]

    def masks_attention(self, cache) -> bool:
        """Does a knockout, or do cuts, rewrite rows of this decode step's attention output?  It then needs q rotated in place
        (the two-launch RoPE + attention form) and a bf16 cache."""
        assert (self.knockout is None and self.cuts is None) or cache.dtype == "bf16", "attention knockout / cuts read a bf16 KV cache"
        return self.knockout is not None or self.cuts is not None


# ================================================================================================
# Host side: validation of the caller's arguments (ValueError before any launch), the device state, the kept rows of a drop
# ================================================================================================
def _need_bf16_kv(what: str, kv_dtype: str) -> None:
    if kv_dtype != "bf16":
        raise ValueError(f"{what} needs the bf16 KV cache (llm_kv_dtype={kv_dtype!r}: the FP8 prefill attends to unrounded "
                         "k / v, so the cache does not hold the keys the attention saw)")


def _check_segments(b: int, n_entries: int, n_positions: int, lo: int, hi: int, prefix: str, note: str) -> None:
    """``segments[b]`` of a readout or a knockout: one id 0..255 per position of prompt b (``lo`` / ``hi``: its smallest / largest id)."""
    if n_entries != n_positions:
        raise ValueError(f"{prefix}segments[{b}] has {n_entries} entries, the prompt of row {b} has {n_positions} positions")
    if n_entries and (lo < 0 or hi > 255):
        raise ValueError(f"{prefix}segments[{b}]: segment ids are 0..255 ({note})")


def _segment_table(ws: Workspace, name: str, segs, max_len: int) -> torch.Tensor:
    """uint8 [n_seqs, max_len] in workspace buffer ``name``: the segment of every cache position, ``IGNORE_SEGMENT`` past the prompt."""
    seg = torch.full((len(segs), max_len), IGNORE_SEGMENT, dtype=torch.uint8)
    for b, sg in enumerate(segs):
        seg[b, :len(sg)] = torch.as_tensor(sg, dtype=torch.uint8)
    seg_d = ws.get(name, tuple(seg.shape), torch.uint8)
    seg_d.copy_(seg, non_blocking=True)
    return seg_d


def check_readout(segments, n_seg: Optional[int], kv_dtype: str, plens: List[int]) -> Tuple[List[torch.Tensor], int]:
    """Host validation of ``prompt_attention(segments=, n_seg=)``: (segments as int64 tensors, the segment count)."""
    _need_bf16_kv("prompt_attention", kv_dtype)
    if len(segments) != len(plens):
        raise ValueError(f"{len(segments)} segment lists for {len(plens)} prompts")
    segs = []
    for b, (sg, n) in enumerate(zip(segments, plens)):
        m, sg = len(sg), torch.as_tensor(sg, dtype=torch.int64).reshape(-1)
        _check_segments(b, m, n, int(sg.min()) if m == n > 0 else 0, int(sg.max()) if m == n > 0 else 0, "", f"{IGNORE_SEGMENT} = counted nowhere")
        segs.append(sg)
    if n_seg is None:
        n_seg = 1 + max(int(sg[sg < IGNORE_SEGMENT].max()) if bool((sg < IGNORE_SEGMENT).any()) else 0 for sg in segs)
    if not 1 <= int(n_seg) <= MAX_READOUT_SEGMENTS:
        raise ValueError(f"{n_seg} segments: the readout kernel sums at most {MAX_READOUT_SEGMENTS}")
    return segs, int(n_seg)


def readout_state(ws: Workspace, cfg, segs: List[torch.Tensor], n_seg: int, lens: List[int], max_len: int, want_probs: bool,
                  device) -> AttnReadout:
    """The validated readout on the device: the segment table padded to the cache length, the prompt lengths, and where the
    launches leave the mass (and the full weights, ``want_probs``: zeroed — the kernel leaves a row's tail untouched)."""
    Bn = len(segs)
    seg_d = _segment_table(ws, "pa_seg", segs, max_len)
    mass = ws.get("pa_mass", (cfg.n_layers, Bn, cfg.n_heads, n_seg), F32)
    probs = ws.get("pa_probs", (cfg.n_layers, Bn, cfg.n_heads, max_len), F32) if want_probs else None
    if probs is not None:
        probs.zero_()
    return AttnReadout(seg_d, _i32(lens, device), mass, probs)


def check_knockout(knockout, cfg, kv_dtype: str, plens: List[int], num_beams: int):
    """Host validation of ``generate(knockout=...)``: everything is a ``ValueError`` raised before any launch.  Returns
    ``(segments as int lists, blocked as sorted tuples, (l0, l1), heads tuple | None)``, or None when every set is empty."""
    if isinstance(knockout, dict):
        unknown = set(knockout) - {"segments", "blocked", "layers", "heads"}
        if unknown or "segments" not in knockout or "blocked" not in knockout:
            raise ValueError("knockout as a dict holds 'segments' and 'blocked', and optionally 'layers' and 'heads'")
        knockout = (knockout["segments"], knockout["blocked"], knockout.get("layers"), knockout.get("heads"))
    try:
        segments, blocked, layers, heads = (tuple(knockout) + (None, None))[:4] if 2 <= len(knockout) <= 4 else (None,) * 4
    except TypeError:
        segments = None
    if segments is None:
        raise ValueError("knockout must be (segments, blocked[, layers[, heads]]) or a dict with those keys")
    if len(segments) != len(plens) or len(blocked) != len(plens):
        raise ValueError(f"knockout: {len(segments)} segment lists and {len(blocked)} blocked sets for {len(plens)} prompts")
    segs, sets = [], []
    for b, (sg, n) in enumerate(zip(segments, plens)):
        sg = [int(x) for x in (sg.tolist() if isinstance(sg, torch.Tensor) else sg)]
        _check_segments(b, len(sg), n, min(sg, default=0), max(sg, default=0), "knockout: ", f"ids >= {MAX_KNOCKOUT_SEGMENTS} are never blocked")
        segs.append(sg)
        bl = tuple(sorted({int(x) for x in blocked[b]}))
        if bl and not (0 <= bl[0] and bl[-1] < MAX_KNOCKOUT_SEGMENTS):
            raise ValueError(f"knockout: blocked[{b}] = {list(bl)}: only segment ids 0..{MAX_KNOCKOUT_SEGMENTS - 1} can be blocked")
        sets.append(bl)
    if layers is None:
        layers = (0, cfg.n_layers)
    try:
        l0, l1 = (int(x) for x in layers)
    except (TypeError, ValueError):
        raise ValueError(f"knockout: layers must be a half-open range (l0, l1), not {layers!r}") from None
    if not 0 <= l0 < l1 <= cfg.n_layers:
        raise ValueError(f"knockout: layer window ({l0}, {l1}) must be a non-empty range inside [0, {cfg.n_layers}]")
    if heads is not None:
        heads = tuple(sorted({int(x) for x in heads}))
        if not heads or heads[0] < 0 or heads[-1] >= cfg.n_heads:
            raise ValueError(f"knockout: head indices {list(heads)} must be a non-empty subset of 0..{cfg.n_heads - 1}")
    for b, (sg, bl) in enumerate(zip(segs, sets)):
        if bl and all(x in bl for x in sg):
            raise ValueError(f"knockout: row {b}: the blocked segments {list(bl)} cover every position of its prompt")
    if not any(sets):
        return None
    _need_bf16_kv("knockout", kv_dtype)
    if num_beams != 1:
        raise ValueError("knockout runs with greedy, sampled and label-constrained decoding, not with beams (num_beams > 1)")
    return segs, sets, (l0, l1), heads


def knockout_state(ws: Workspace, cfg, knockout, max_len: int) -> Knockout:
    """The validated knockout on the device, in graph-visible workspace buffers refilled on every call: the segment table
    padded to the cache length, the listed rows (non-empty sets) and their per-head bit sets."""
    segs, sets, layers, heads = knockout
    listed = tuple(b for b, bl in enumerate(sets) if bl)
    on = set(range(cfg.n_heads) if heads is None else heads)
    bits = []
    for b in listed:
        m = sum(1 << g for g in sets[b])
        m -= (1 << 32) if m >= (1 << 31) else 0           # the u32 bit set in an int32 tensor
        bits.append([m if h in on else 0 for h in range(cfg.n_heads)])
    seg_d = _segment_table(ws, "gen_ko_seg", segs, max_len)
    blk_d = ws.get("gen_ko_blocked", (len(listed), cfg.n_heads), I32)
    rows_d = ws.get("gen_ko_rows", (len(listed),), I32)
    blk_d.copy_(torch.tensor(bits, dtype=I32), non_blocking=True)
    rows_d.copy_(torch.tensor(listed, dtype=I32), non_blocking=True)
    return Knockout(seg_d, blk_d, rows_d, listed, layers)


def _cut_pairs(pairs, n_prompts: int):
    """``pairs`` of a ``cuts`` dict as one {query segment: u32 bit set of key segments} per prompt: one list of (q_seg, k_seg)
    for all prompts, or one such list per prompt."""
    def one(lst, where):
        K = {}
        try:
            lst = [(int(a), int(b)) for a, b in lst]
        except (TypeError, ValueError):
            raise ValueError(f"cuts: {where} must be a list of (q_seg, k_seg) pairs, not {lst!r}") from None
        for a, b in lst:
            if not (0 <= a < MAX_CUT_SEGMENTS and 0 <= b < MAX_CUT_SEGMENTS):
                raise ValueError(f"cuts: {where} holds the pair ({a}, {b}): both segment ids of a pair are 0..{MAX_CUT_SEGMENTS - 1}")
            K[a] = K.get(a, 0) | (1 << b)
        return K
    try:
        items = list(pairs)
    except TypeError:
        raise ValueError(f"cuts: pairs must be a list of (q_seg, k_seg) pairs, or one such list per prompt, not {pairs!r}") from None
    is_int = lambda x: isinstance(x, int) and not isinstance(x, bool)
    if all(isinstance(e, (tuple, list)) and len(e) == 2 and is_int(e[0]) and is_int(e[1]) for e in items):
        return [one(items, "pairs")] * n_prompts
    if len(items) != n_prompts:
        raise ValueError(f"cuts: pairs is neither one list of (q_seg, k_seg) pairs nor one list per prompt ({len(items)} lists for "
                         f"{n_prompts} prompts)")
    return [one(lst, f"pairs[{b}]") for b, lst in enumerate(items)]


def check_cuts(cuts, cfg, kv_dtype: str, plens: List[int], num_beams: int, knockout=None, patch=None, head_patch=None):
    """Host validation of ``generate(cuts=...)``: everything is a ``ValueError`` raised before any launch.  Returns a dict —
    the arguments in one form (``segments`` as int64 arrays, ``pairs`` one list per prompt, ``generated`` one id per prompt,
    ``layers`` (l0, l1), ``heads`` a tuple or None: itself a valid ``cuts``) and what follows from them: ``entries[b]`` the listed
    positions of prompt b and their bit sets K(seg[p]), two int64 arrays, ``gen[b]`` the bit set of prompt b's generated rows (0:
    untouched) — or None when no row is listed and no generated row cuts anything: the call is then the plain one.

    Position p of prompt b is listed iff at least one key j <= p has seg[j] in K(seg[p])."""
    if not isinstance(cuts, dict):
        raise ValueError(f"cuts must be a dict with the keys {CUT_KEYS}")
    unknown = set(cuts) - set(CUT_KEYS)
    if unknown or "segments" not in cuts or "pairs" not in cuts:
        raise ValueError(f"cuts holds 'segments' and 'pairs', and optionally 'layers', 'heads' and 'generated' (unknown keys: {sorted(unknown)})")
    segments, n = cuts["segments"], len(plens)
    if len(segments) != n:
        raise ValueError(f"cuts: {len(segments)} segment lists for {n} prompts")
    segs = []
    for b, (sg, m) in enumerate(zip(segments, plens)):
        try:
            sg = np.asarray(sg.cpu() if isinstance(sg, torch.Tensor) else sg).astype(np.int64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"cuts: segments[{b}] must be a list of segment ids") from None
        _check_segments(b, len(sg), m, int(sg.min()) if len(sg) else 0, int(sg.max()) if len(sg) else 0, "cuts: ",
                        f"ids >= {MAX_CUT_SEGMENTS} are never cut")
        segs.append(sg)
    Ks = _cut_pairs(cuts["pairs"], n)
    layers, heads, generated = cuts.get("layers"), cuts.get("heads"), cuts.get("generated")
    if layers is None:
        layers = (0, cfg.n_layers)
    try:
        l0, l1 = (int(x) for x in layers)
    except (TypeError, ValueError):
        raise ValueError(f"cuts: layers must be a half-open range (l0, l1), not {layers!r}") from None
    if not 0 <= l0 < l1 <= cfg.n_layers:
        raise ValueError(f"cuts: layer window ({l0}, {l1}) must be a non-empty range inside [0, {cfg.n_layers}]")
    if heads is not None:
        try:
            heads = tuple(sorted({int(x) for x in heads}))
        except (TypeError, ValueError):
            raise ValueError(f"cuts: heads must be None or a list of query-head indices, not {cuts['heads']!r}") from None
        if not heads or heads[0] < 0 or heads[-1] >= cfg.n_heads:
            raise ValueError(f"cuts: head indices {list(heads)} must be a non-empty subset of 0..{cfg.n_heads - 1}")
    if generated is None:
        gen_ids = [int(sg[-1]) if len(sg) else IGNORE_SEGMENT for sg in segs]
    else:
        try:
            gen_ids = [int(generated)] * n if isinstance(generated, int) and not isinstance(generated, bool) else [int(x) for x in generated]
        except (TypeError, ValueError):
            raise ValueError(f"cuts: generated must be None, a segment id or one id per prompt, not {generated!r}") from None
        if len(gen_ids) != n or not all(0 <= g <= 255 for g in gen_ids):
            raise ValueError(f"cuts: generated = {generated!r}: one segment id 0..255 for all prompts, or one per prompt ({n})")
    entries, gen = [], []
    for b, (sg, K) in enumerate(zip(segs, Ks)):
        low = sg < MAX_CUT_SEGMENTS
        listed, masks = np.zeros(len(sg), dtype=bool), np.zeros(len(sg), dtype=np.int64)
        for s, m in K.items():
            cut = np.cumsum(low & ((m >> np.where(low, sg, 0)) & 1 == 1))        # keys j <= p that segment s does not read
            mine = (sg == s) & (cut > 0)
            blind = mine & (cut == np.arange(1, len(sg) + 1))
            if blind.any():
                raise ValueError(f"cuts: prompt {b}, position {int(np.argmax(blind))} (segment {s}): the cut segments "
                                 f"{[g for g in range(MAX_CUT_SEGMENTS) if (m >> g) & 1]} cover every key it could read")
            listed |= mine
            masks[mine] = m
        entries.append((np.nonzero(listed)[0], masks[listed]))
        seen = sum(1 << int(g) for g in np.unique(sg[low]))
        gen.append(K.get(gen_ids[b], 0) & seen)       # a key segment the prompt does not hold is no cut
    if not any(len(pos) for pos, _ in entries) and not any(gen):
        return None
    _need_bf16_kv("cuts", kv_dtype)
    if num_beams != 1:
        raise ValueError("cuts run with greedy, sampled and label-constrained decoding, not with beams (num_beams > 1)")
    if knockout is not None or patch is not None or head_patch is not None:
        raise ValueError("cuts together with knockout, patch or head_patch is not supported")
    pairs = [[(a, g) for a, m in sorted(K.items()) for g in range(MAX_CUT_SEGMENTS) if (m >> g) & 1] for K in Ks]
    return dict(segments=segs, pairs=pairs, generated=gen_ids, entries=tuple(entries), gen=gen, layers=(l0, l1), heads=heads)


def cuts_state(ws: Workspace, cfg, cuts, max_len: int) -> Cuts:
    """The validated cuts: the per-sequence host lists of listed positions and bit sets, and on the device, in graph-visible
    workspace buffers refilled on every call, the segment table padded to the cache length, the head switch, and the decode
    steps' state for the sequences whose generated rows cut something (the knockout's operands)."""
    heads, gen = cuts["heads"], cuts["gen"]
    seg_d = _segment_table(ws, "gen_ct_seg", [sg.astype(np.uint8) for sg in cuts["segments"]], max_len)
    head_on = None
    if heads is not None and len(heads) < cfg.n_heads:
        head_on = ws.get("gen_ct_heads", (cfg.n_heads,), torch.uint8)
        head_on.copy_(torch.tensor([int(h in heads) for h in range(cfg.n_heads)], dtype=torch.uint8), non_blocking=True)
    R = B.load_library().icl_attn_cut_tile_rows(cfg.n_heads, cfg.kv_heads, cfg.head_dim)      # a host query of the library, no launch
    if R <= 0:
        raise ValueError(f"cuts: no row-tile attention form for n_heads={cfg.n_heads}, n_kv_heads={cfg.kv_heads}, head_dim={cfg.head_dim}")
    state = Cuts(seg_d, cuts["entries"], cuts["layers"], cfg.n_layers, R, head_on)
    listed = tuple(b for b, m in enumerate(gen) if m)
    if listed:
        on = set(range(cfg.n_heads) if heads is None else heads)
        bits = [[(gen[b] - (1 << 32) if gen[b] >= (1 << 31) else gen[b]) if h in on else 0 for h in range(cfg.n_heads)] for b in listed]
        state.gen_listed = listed
        state.gen_blocked = ws.get("gen_ct_blocked", (len(listed), cfg.n_heads), I32)
        state.gen_row_seq = ws.get("gen_ct_rows", (len(listed),), I32)
        state.gen_blocked.copy_(torch.tensor(bits, dtype=I32), non_blocking=True)
        state.gen_row_seq.copy_(torch.tensor(listed, dtype=I32), non_blocking=True)
    return state


def _patch_options(d: dict, n_prompts: int, what: str):
    """``mode``, ``steps``, ``alpha`` and ``rows`` of a ``patch`` / ``head_patch`` dict, validated: (mode, steps, alpha as a float,
    the rows as an ascending list — all prompts for None)."""
    mode, steps = d.get("mode", "replace"), d.get("steps", "prompt")
    if mode not in ("replace", "add"):
        raise ValueError(f"{what}: mode must be 'replace' or 'add', not {mode!r}")
    if steps not in ("prompt", "all"):
        raise ValueError(f"{what}: steps must be 'prompt' or 'all', not {steps!r}")
    try:
        alpha = float(d.get("alpha", 1.0))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: alpha must be a finite number, not {d.get('alpha')!r}") from None
    if not math.isfinite(alpha):
        raise ValueError(f"{what}: alpha must be finite, not {alpha}")
    rows = d.get("rows")
    if rows is None:
        rows = list(range(n_prompts))
    else:
        try:
            rows = [int(b) for b in rows]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: rows must be None or a list of prompt indices, not {d.get('rows')!r}") from None
        if len(set(rows)) != len(rows):
            raise ValueError(f"{what}: rows {rows} lists a prompt twice")
        if rows and not (0 <= min(rows) and max(rows) < n_prompts):
            raise ValueError(f"{what}: rows {rows} outside 0..{n_prompts - 1}")
        rows = sorted(rows)
    return mode, steps, alpha, rows


def check_patch(patch, cfg, n_prompts: int, num_beams: int, knockout):
    """Host validation of ``generate(patch=...)``: everything is a ``ValueError`` raised before any launch.  Returns the
    patch as a dict of all ``PATCH_KEYS`` — ``vectors`` f32 [n_prompts or 1, hidden], ``rows`` an ascending list — or None
    when ``rows`` is empty."""
    if not isinstance(patch, dict):
        raise ValueError(f"patch must be a dict with the keys {PATCH_KEYS}")
    unknown = set(patch) - set(PATCH_KEYS)
    if unknown or "site" not in patch or "vectors" not in patch:
        raise ValueError(f"patch holds 'site' and 'vectors', and optionally 'mode', 'alpha', 'rows' and 'steps' (unknown: {sorted(unknown)})")
    site, vec = patch["site"], patch["vectors"]
    if isinstance(site, bool) or not isinstance(site, int) or not 0 <= site <= cfg.n_layers:
        raise ValueError(f"patch: site {site!r} must be an integer in 0..{cfg.n_layers} (n_layers = the last layer's output)")
    if not isinstance(vec, torch.Tensor) or vec.dtype != F32:
        raise ValueError("patch: vectors must be a float32 tensor")
    if vec.dim() == 1:
        vec = vec[None]
    if vec.dim() != 2 or vec.shape[1] != cfg.hidden or vec.shape[0] not in (1, n_prompts):
        raise ValueError(f"patch: vectors of shape {tuple(patch['vectors'].shape)}: [{n_prompts}, {cfg.hidden}] (one per prompt), "
                         f"[1, {cfg.hidden}] or [{cfg.hidden}] (shared)")
    mode, steps, alpha, rows = _patch_options(patch, n_prompts, "patch")
    if num_beams != 1:
        raise ValueError("patch runs with greedy, sampled and label-constrained decoding, not with beams (num_beams > 1)")
    if knockout is not None:
        raise ValueError("patch together with knockout is not supported")
    if not rows:
        return None
    return dict(site=site, vectors=vec, mode=mode, alpha=alpha, rows=rows, steps=steps)


def patch_state(ws: Workspace, cfg, patch) -> ResidPatch:
    """The validated patch on the device, in graph-visible workspace buffers refilled on every call: the listed rows'
    vectors (one row of the buffer when the vector is shared) and the listed sequences."""
    vec, rows = patch["vectors"], patch["rows"]
    if vec.shape[0] != 1:
        vec = vec[torch.tensor(rows, device=vec.device)]
    vec_d = ws.get("gen_rp_vec", (vec.shape[0], cfg.hidden), F32)
    rows_d = ws.get("gen_rp_rows", (len(rows),), I32)
    vec_d.copy_(vec, non_blocking=True)
    rows_d.copy_(torch.tensor(rows, dtype=I32), non_blocking=True)
    return ResidPatch(vec_d, rows_d, tuple(rows), patch["site"], patch["mode"], patch["alpha"], patch["steps"])


def check_head_patch(hp, cfg, n_prompts: int, num_beams: int, knockout, patch):
    """Host validation of ``generate(head_patch=...)``: everything is a ``ValueError`` raised before any launch.  Returns the
    patch as a dict of all ``HEAD_PATCH_KEYS`` — ``heads`` a list of (layer, head) as given, ``vectors`` f32 [n_prompts or 1,
    n_pairs, head_dim] in that order, ``rows`` an ascending list — or None when ``rows`` is empty."""
    if not isinstance(hp, dict):
        raise ValueError(f"head_patch must be a dict with the keys {HEAD_PATCH_KEYS}")
    unknown = set(hp) - set(HEAD_PATCH_KEYS)
    if unknown or "heads" not in hp or "vectors" not in hp:
        raise ValueError("head_patch holds 'heads' and 'vectors', and optionally 'mode', 'alpha', 'rows' and 'steps' "
                         f"(unknown: {sorted(unknown)})")
    pairs = check_head_pairs(hp["heads"], cfg, "head_patch")
    vec, D = hp["vectors"], cfg.head_dim
    if not isinstance(vec, torch.Tensor) or vec.dtype != F32:
        raise ValueError("head_patch: vectors must be a float32 tensor")
    if vec.dim() == 2:
        vec = vec[None]
    if vec.dim() != 3 or tuple(vec.shape[1:]) != (len(pairs), D) or vec.shape[0] not in (1, n_prompts):
        raise ValueError(f"head_patch: vectors of shape {tuple(hp['vectors'].shape)}: [{n_prompts}, {len(pairs)}, {D}] (one block per "
                         f"prompt), [1, {len(pairs)}, {D}] or [{len(pairs)}, {D}] (shared), in the order of heads")
    mode, steps, alpha, rows = _patch_options(hp, n_prompts, "head_patch")
    if num_beams != 1:
        raise ValueError("head_patch runs with greedy, sampled and label-constrained decoding, not with beams (num_beams > 1)")
    if knockout is not None or patch is not None:
        raise ValueError("head_patch together with knockout or with patch is not supported")
    if not rows:
        return None
    return dict(heads=pairs, vectors=vec, mode=mode, alpha=alpha, rows=rows, steps=steps)


def check_head_pairs(heads, cfg, what: str) -> List[Tuple[int, int]]:
    """(layer, head) pairs as a list of int tuples: inside [0, n_layers) x [0, n_heads), non-empty, none given twice."""
    try:
        pairs = [(int(l), int(h)) for l, h in heads]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: heads must be a list of (layer, head) pairs, not {heads!r}") from None
    if not pairs:
        raise ValueError(f"{what}: heads is empty")
    bad = [p for p in pairs if not (0 <= p[0] < cfg.n_layers and 0 <= p[1] < cfg.n_heads)]
    if bad:
        raise ValueError(f"{what}: pairs {bad} outside [0, {cfg.n_layers}) x [0, {cfg.n_heads})")
    if len(set(pairs)) != len(pairs):
        raise ValueError(f"{what}: heads {pairs} holds a pair twice")
    return pairs


def head_patch_state(ws: Workspace, cfg, hp) -> HeadPatch:
    """The validated head patch on the device, in graph-visible workspace buffers refilled on every call: the head indices
    sorted by (layer, head), the listed rows' vectors permuted to that order (one block when they are shared) and the listed
    sequences."""
    pairs, vec, rows = hp["heads"], hp["vectors"], hp["rows"]
    order = sorted(range(len(pairs)), key=lambda i: pairs[i])
    vec = vec[:, torch.tensor(order, device=vec.device)]
    if vec.shape[0] != 1:
        vec = vec[torch.tensor(rows, device=vec.device)]
    layers, p0 = [], 0
    for p1 in range(1, len(order) + 1):
        if p1 == len(order) or pairs[order[p1]][0] != pairs[order[p0]][0]:
            layers.append((pairs[order[p0]][0], p0, p1))
            p0 = p1
    vec_d = ws.get("gen_hp_vec", (vec.shape[0], len(pairs), cfg.head_dim), F32)
    heads_d = ws.get("gen_hp_heads", (len(pairs),), I32)
    rows_d = ws.get("gen_hp_rows", (len(rows),), I32)
    vec_d.copy_(vec, non_blocking=True)
    heads_d.copy_(torch.tensor([pairs[i][1] for i in order], dtype=I32), non_blocking=True)
    rows_d.copy_(torch.tensor(rows, dtype=I32), non_blocking=True)
    return HeadPatch(vec_d, heads_d, rows_d, tuple(rows), tuple(layers), hp["mode"], hp["alpha"], hp["steps"])


def keep_cut_rows(cuts, keep: List[int]):
    """``overlong="drop"``: validated cuts as the ``cuts`` argument of the call over the prompts ``keep``."""
    if cuts is None:
        return None
    return dict(segments=[cuts["segments"][b] for b in keep], pairs=[cuts["pairs"][b] for b in keep], layers=cuts["layers"],
                heads=cuts["heads"], generated=[cuts["generated"][b] for b in keep])


def keep_rows(knockout, patch, keep: List[int], head_patch=None):
    """``overlong="drop"``: a validated knockout, patch and head patch for the call over the prompts ``keep`` — the surviving
    rows' entries and vectors, a patch's rows under the indices they have among the survivors."""
    if head_patch is not None:
        vec = head_patch["vectors"]
        head_patch = dict(head_patch, vectors=vec if vec.shape[0] == 1 else vec[torch.tensor(keep, device=vec.device)],
                          rows=[keep.index(b) for b in head_patch["rows"] if b in keep])
    if knockout is not None:
        knockout = ([knockout[0][b] for b in keep], [knockout[1][b] for b in keep]) + tuple(knockout[2:])
    if patch is not None:
        vec = patch["vectors"]
        patch = dict(patch, vectors=vec if vec.shape[0] == 1 else vec[torch.tensor(keep, device=vec.device)],
                     rows=[keep.index(b) for b in patch["rows"] if b in keep])
    return knockout, patch, head_patch
