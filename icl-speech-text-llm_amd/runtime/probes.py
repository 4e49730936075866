"""Probes of the deciding rows of the LLM decoder — the last prompt row of every sequence and the rows generated after it:

  the prompt-attention readout   ``AttnReadout``          icl_attn_segmass_bf16         where the row looks, per prompt segment
                                                          icl_attn_segflow_bf16         (``flow``) where EVERY prompt row looks, per segment pair
  attention knockout             ``Knockout``             icl_attn_decode_masked_bf16   the row attends as if segments were absent
  residual capture / patching    a tensor, ``ResidPatch`` icl_resid_rows_f32            the row's residual stream, read and written
  head-output capture / patching a tensor, ``HeadPatch``  icl_head_rows_bf16            what single heads hand to o_proj, read and written

and of ANY prompt row: attention cuts between prompt segments, ``Cuts`` (icl_attn_cut_rows_bf16; in the decode steps a ``Knockout``).

``check_probes`` validates the probe arguments of ``generate`` into one ``ProbeArgs``, which re-slices itself to the kept rows of a
drop (``kept``) and builds the device state (``state``): ``Probes``, the one bundle handed between runtime/salmonn.py and
runtime/engines.py.  The probes share their parts: ``RowList`` (the sequences a probe lists), one ``rows`` for a
prefill chunk, one builder of the per-head bit sets, one base of the two patches.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, fields, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import binding as B
from .engines import BF16, F32, I32, Workspace, _i32

MAX_READOUT_SEGMENTS = 32      # icl_attn_segmass_bf16: one thread per (head of a K/V group, segment)
MAX_KNOCKOUT_SEGMENTS = 32     # icl_attn_decode_masked_bf16: one bit of a u32 per segment; ids >= 32 are never blocked
MAX_CUT_SEGMENTS = 32          # icl_attn_cut_rows_bf16: the same bit set per listed row
IGNORE_SEGMENT = 255           # a segment id that is counted nowhere and never blocked, whatever n_seg is
KNOCKOUT_KEYS = ("segments", "blocked", "layers", "heads")          # of each dict: the required keys first
CUT_KEYS = ("segments", "pairs", "layers", "heads", "generated")
PATCH_KEYS = ("site", "vectors", "mode", "alpha", "rows", "steps")
HEAD_PATCH_KEYS = ("heads", "vectors", "mode", "alpha", "rows", "steps")


# ================================================================================================
# Device state: what a launch reads, and the launch
# ================================================================================================
@dataclass
class AttnReadout:
    """Where a prefill leaves the prompt-attention readout of its sequences, all on the device: ``seg`` uint8 [n_seqs, >= cache
    max_len] the segment of every prompt position (>= n_seg: counted nowhere), ``lens`` int32 [n_seqs] the prompt lengths,
    ``mass`` f32 [n_layers, n_seqs, n_heads, n_seg] and ``probs`` None or f32 [n_layers, n_seqs, n_heads, >= max_len] (written).
    ``flow``: None, or f32 [n_layers, n_seqs, n_heads, n_seg, n_seg] (written) — the segment-to-segment flow of ALL prompt rows
    (icl_attn_segflow_bf16), which needs every query of every layer: a prefill does not trim its last layer for such a readout
    (``Probes.reads_every_row``).  ``cu`` / ``max_seqlen``: what the flow launch needs of the prefill in progress
    (``start_prefill``): int32 [n_seqs + 1] the first packed row of every sequence, and the longest sequence."""
    seg: torch.Tensor
    lens: torch.Tensor
    mass: torch.Tensor
    probs: Optional[torch.Tensor] = None
    flow: Optional[torch.Tensor] = None
    cu: Optional[torch.Tensor] = None
    max_seqlen: int = 0

    def rows(self, b0: int, b1: int) -> "AttnReadout":
        """The readout of sequences b0 .. b1-1 (views), for a prefill over that chunk of the batch (``KVCache.rows``)."""
        return AttnReadout(self.seg[b0:b1], self.lens[b0:b1], self.mass[:, b0:b1],
                           None if self.probs is None else self.probs[:, b0:b1],
                           None if self.flow is None else self.flow[:, b0:b1])

    def start_prefill(self, seq_lens: List[int], cu_h: List[int]) -> None:
        if self.flow is not None:
            self.cu, self.max_seqlen = _i32(cu_h, self.flow.device), max(seq_lens)

    def launch_flow(self, layer: int, q: torch.Tensor, kc: torch.Tensor, cfg, max_len: int) -> None:
        """``q``: the packed rotated query rows of the prefill in progress, all of them."""
        B.attn_segflow(q, self.cu, kc, self.seg, self.flow[layer], cfg.n_heads, cfg.head_dim, max_len, self.max_seqlen,
                       cfg.head_dim ** -0.5, n_kv_heads=cfg.kv_heads)

    def launch(self, layer: int, q: torch.Tensor, q_rows: Optional[torch.Tensor], kc: torch.Tensor, cfg, max_len: int) -> None:
        B.attn_segmass(q, kc, self.lens, self.seg, self.mass[layer], cfg.n_heads, cfg.head_dim, max_len, cfg.head_dim ** -0.5,
                       n_kv_heads=cfg.kv_heads, q_rows=q_rows, probs=None if self.probs is None else self.probs[layer])


@dataclass
class RowList:
    """The sequences a probe lists, ascending and distinct: ``seqs`` on the host, ``dev`` int32 [n] the same on the device — row b
    of a decode step's or of the gathered last rows' operands is sequence b's.  ``last``: the sequences' last packed rows in the
    prefill in progress (``Probes.start_prefill``), where the deciding row of a sequence is the last of its packed rows."""
    seqs: Tuple[int, ...]
    dev: torch.Tensor
    last: Optional[torch.Tensor] = None

    @staticmethod
    def filled(buf: torch.Tensor, seqs) -> "RowList":
        buf.copy_(torch.tensor(seqs, dtype=I32), non_blocking=True)
        return RowList(tuple(seqs), buf)

    def rows(self, b0: int, b1: int):
        """Of the listed sequences, those of the chunk b0 .. b1-1: None when there is none, else (first entry, end entry, their
        list with the sequences relative to b0)."""
        lo = sum(1 for s in self.seqs if s < b0)
        hi = sum(1 for s in self.seqs if s < b1)
        if lo == hi:
            return None
        if b0 == 0 and hi == len(self.seqs):
            return lo, hi, self
        sub = tuple(s - b0 for s in self.seqs[lo:hi])
        return lo, hi, RowList(sub, _i32(sub, self.dev.device))

    def start_prefill(self, cu_h: List[int]) -> None:
        self.last = _i32([cu_h[b + 1] - 1 for b in self.seqs], self.dev.device)

    def at(self, packed: bool) -> torch.Tensor:
        """The listed sequences' deciding rows: of the packed rows of a prefill, else row b for sequence b."""
        return self.last if packed else self.dev


class _ListedRows:
    """A probe of the sequences in its ``listed``; ``_chunk`` names what else a prefill chunk gets as views."""

    def rows(self, b0: int, b1: int):
        """The probe of sequences b0 .. b1-1 (views; sequence ids relative to b0), for a prefill over that chunk of the batch
        (``KVCache.rows``); None when the chunk lists no row."""
        part = self.listed.rows(b0, b1)
        if part is None:
            return None
        lo, hi, listed = part
        return replace(self, listed=listed, **self._chunk(b0, b1, lo, hi))


class _LayerWindow:
    def covers(self, layer: int) -> bool:
        return self.layers[0] <= layer < self.layers[1]


@dataclass
class Knockout(_ListedRows, _LayerWindow):
    """Attention knockout, all on the device: in decoder layers ``layers[0] .. layers[1] - 1`` the LAST prompt row and every
    generated row of the listed sequences attend as if the keys of their blocked segments were not there
    (icl_attn_decode_masked_bf16 rewrites those rows of the attention output after the layer's ordinary attention launch).
    ``seg`` uint8 [n_seqs, >= cache max_len]: the segment of every cache position, 255 past the prompt (generated positions are
    always visible); ``blocked`` int32 [n_listed, n_heads]: bit g of a (listed row, query head) = segment g is not read;
    ``listed``: the listed sequences.  The runtime keeps all three in graph-visible workspace buffers and refills them on every
    call, so ``uid`` — what a captured decode graph bakes in besides those pointers: the number of listed rows (a grid size) and
    the layer window — keys the decode graphs."""
    seg: torch.Tensor
    blocked: torch.Tensor
    listed: RowList
    layers: Tuple[int, int]
    every_step = True

    @property
    def uid(self):
        return ("knockout", len(self.listed.seqs), self.layers[0], self.layers[1])

    def _chunk(self, b0, b1, lo, hi):
        return dict(seg=self.seg[b0:b1], blocked=self.blocked[lo:hi])

    def launch(self, q: torch.Tensor, att: torch.Tensor, row_q: torch.Tensor, kc, vc, lens: torch.Tensor, cfg, max_len: int) -> None:
        """Rewrite rows ``row_q`` (int32 [n_listed]) of ``att`` from the same rows of ``q`` (rotated) over the bf16 cache."""
        B.attn_decode_masked(q, kc, vc, att, lens, self.seg, self.blocked, self.listed.dev, row_q, cfg.n_heads, cfg.head_dim, max_len,
                             cfg.head_dim ** -0.5, n_kv_heads=cfg.kv_heads)


@dataclass
class _RowsPatch(_ListedRows):
    """What the two patches of the deciding rows share: the LAST prompt row of the listed sequences — and with ``steps == "all"``
    every generated row — is replaced by its vectors, or gets ``alpha`` times its vectors added.  ``vectors`` f32 [n_listed, ...],
    or [1, ...]: one for all listed rows.  The runtime keeps the tensors in graph-visible workspace buffers and refills them on
    every call, so ``uid`` — what a captured decode graph bakes in besides those pointers: the number of listed rows (a grid
    size), whether the vectors are shared (a leading dimension), where the patch launches, mode, steps and alpha, a by-value
    kernel argument — keys the decode graphs."""
    vectors: torch.Tensor
    listed: RowList
    mode: str
    alpha: float
    steps: str

    @property
    def every_step(self) -> bool:
        return self.steps == "all"

    def _uid(self, name: str, where):
        return (name, len(self.listed.seqs), int(self.vectors.shape[0]), where, self.mode, self.steps, float(self.alpha))

    def _chunk(self, b0, b1, lo, hi):
        return dict(vectors=self.vectors if self.vectors.shape[0] == 1 else self.vectors[lo:hi])


@dataclass
class ResidPatch(_RowsPatch):
    """Residual-stream patching at the deciding rows (icl_resid_rows_f32) at site ``site`` (0 .. n_layers - 1: the input of that
    decoder layer, before its norm; n_layers: the output of the last layer, before the final norm).  ``vectors`` f32 [n_listed or
    1, hidden]."""
    site: int

    @property
    def uid(self):
        return self._uid("resid_patch", self.site)

    def operands(self) -> dict:
        return dict(vec=self.vectors, mode=self.mode, alpha=self.alpha)


@dataclass
class HeadPatch(_RowsPatch):
    """Attention-head output patching at the deciding rows (icl_head_rows_bf16): in the attention output of a decoder layer — the
    operand of its o_proj — the selected heads are patched.  ``heads`` int32 [n_pairs]: the head indices of the (layer, head)
    pairs, sorted by layer and head; ``layers``: (layer, first pair, end pair) of every layer with a selected head, ascending —
    in ``uid`` with their head counts, grid sizes and offsets into the buffers; ``vectors`` f32 [n_listed or 1, n_pairs,
    head_dim] in that order of pairs."""
    heads: torch.Tensor
    layers: Tuple[Tuple[int, int, int], ...]

    @property
    def uid(self):
        return self._uid("head_patch", tuple((l, p1 - p0) for l, p0, p1 in self.layers))

    def pairs(self, layer: int) -> Optional[Tuple[int, int]]:
        """(first pair, end pair) of ``layer``, or None: no head of the layer is selected."""
        return next(((p0, p1) for l, p0, p1 in self.layers if l == layer), None)

    def operands(self, layer: int) -> dict:
        p0, p1 = self.pairs(layer)
        return dict(heads=self.heads[p0:p1], vec=self.vectors[:, p0:p1], mode=self.mode, alpha=self.alpha)


def _as_i32_bits(masks) -> np.ndarray:
    """u32 bit sets as the int32 values that hold them (bit 31: the sign)."""
    m = np.asarray(masks, dtype=np.int64)
    return np.where(m >= 1 << 31, m - (1 << 32), m)


@dataclass
class Cuts(_LayerWindow):
    """Attention cuts between prompt segments: in decoder layers ``layers[0] .. layers[1] - 1`` and the query heads that are on, a
    query of segment s at ANY prompt position attends as if the keys of the segments K(s) cut for it were absent
    (icl_attn_cut_rows_bf16 rewrites the listed rows of the attention output after the layer's ordinary attention launch).
    ``entries[b]``: the listed positions of sequence b, ascending, and their u32 bit sets, two int64 arrays ``(positions, masks)``
    — on the HOST: a prefill builds its tile tables from them (``tile_tables``), ``tile_rows`` rows of one sequence per tile.  ``seg`` uint8
    [n_seqs, >= cache max_len]: the segment of every cache position, 255 past the prompt (generated positions are always
    visible); ``head_on``: None (all heads) or uint8 [n_heads].  ``step``: the decode steps' state, a ``Knockout`` over ``seg`` of
    the sequences whose generated rows cut something, or None.  ``seg``, ``head_on`` and the decode state live in graph-visible
    workspace buffers refilled on every call, so ``uid`` — what a captured decode graph bakes in besides those pointers: the
    number of sequences listed in the decode steps (a grid size) and the layer window — keys the decode graphs; nothing of the
    prefill's tables reaches a decode graph."""
    seg: torch.Tensor
    entries: Tuple[Tuple[np.ndarray, np.ndarray], ...]
    layers: Tuple[int, int]
    n_layers: int
    tile_rows: int
    head_on: Optional[torch.Tensor] = None
    step: Optional[Knockout] = None

    @property
    def every_step(self) -> bool:
        return self.step is not None

    @property
    def uid(self):
        return ("cuts", 0 if self.step is None else len(self.step.listed.seqs), self.layers[0], self.layers[1])

    def rows(self, b0: int, b1: int) -> Optional["Cuts"]:
        """The cuts of sequences b0 .. b1-1 (views; sequence ids relative to b0), for a prefill over that chunk of the batch
        (``KVCache.rows``); None when the chunk lists no row.  The decode state stays behind: a prefill does not read it."""
        if not any(len(pos) for pos, _ in self.entries[b0:b1]):
            return None
        return Cuts(self.seg[b0:b1], self.entries[b0:b1], self.layers, self.n_layers, self.tile_rows, self.head_on)

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
            blocked.append(np.concatenate([_as_i32_bits(msk), pad]))
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
    # host tables of the prefill in progress (``start_prefill``): the sequences' last packed rows and the prompt lengths as the
    # masked launch's key counts, int32 on the device (the listed sequences' last packed rows: their ``RowList.last``) ...
    _last: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    _key_counts: Optional[torch.Tensor] = field(default=None, init=False, repr=False)
    # ... and what the cuts' tile tables are built from and kept in: (prompt lengths, first packed rows), tables by (last rows
    # only, packed rows)
    _ct_prefill: Optional[tuple] = field(default=None, init=False, repr=False)
    _ct_tables: dict = field(default_factory=dict, init=False, repr=False)

    def _parts(self) -> dict:
        """The probes that are there, by field name."""
        return {f.name: getattr(self, f.name) for f in fields(self) if f.init and getattr(self, f.name) is not None}

    def _or_none(self) -> Optional["Probes"]:
        return self if self._parts() else None

    def rows(self, b0: int, b1: int) -> Optional["Probes"]:
        """The bundle of a prefill over sequences b0 .. b1-1.  A probe that lists no row of the chunk is absent from it, and a
        bundle with nothing left is None: the chunk then launches what it launches without probes."""
        return Probes(**{k: p[b0:b1] if isinstance(p, torch.Tensor) else p.rows(b0, b1) for k, p in self._parts().items()})._or_none()

    @property
    def reads_every_row(self) -> bool:
        """Does a probe read the queries of EVERY prompt row in every layer (the readout's ``flow``)?  ``LlamaHIP.prefill`` then
        keeps its last layer at full height and gathers the last rows after it — bit-identical for those rows, the trim's own
        contract."""
        return self.readout is not None and self.readout.flow is not None

    def _every_step(self) -> dict:
        """The probes that launch in every decode step: the knockout, a patch and a head patch of every step, and cuts whose
        generated rows cut something."""
        return {k: p for k, p in self._parts().items() if getattr(p, "every_step", False)}

    def decode_steps(self) -> Optional["Probes"]:
        """The bundle of the decode steps; None when the steps are the plain ones."""
        return Probes(**self._every_step())._or_none()

    def graph_key(self) -> tuple:
        """What a captured decode loop bakes in of its probes besides pointers: appended to the graph key of the plain call."""
        return tuple(p.uid for p in self._every_step().values())

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
        self._last = last_idx
        self._key_counts = None if self.knockout is None else _i32(seq_lens, last_idx.device)
        if self.readout is not None:
            self.readout.start_prefill(seq_lens, cu_h)
        for p in self._parts().values():
            if isinstance(p, _ListedRows):
                p.listed.start_prefill(cu_h)

    # ---- the three hook points of a layer.  ``packed``: the rows of h / q / att are the packed rows of a prefill, where the
    # deciding row of a sequence is its last one; otherwise row b is sequence b's (a decode step, the gathered last rows) ----
    def _capture_and_patch(self, cap: Optional[torch.Tensor], patch: Optional[_RowsPatch], packed: bool, device, launch) -> bool:
        """``cap`` receives the deciding row of every sequence and ``patch`` rewrites those of its listed sequences, through
        ``launch(rows, capture, patch)``.  One launch does both when the patch lists every sequence; a patch of some sequences
        next to a capture of all is a capture launch and then a patch launch.  True when rows were rewritten."""
        if cap is not None:
            n = cap.shape[0]
            all_rows = self._last if packed else _i32(list(range(n)), device)
            if patch is not None and patch.listed.seqs == tuple(range(n)):
                launch(all_rows, cap, patch)
                return True
            launch(all_rows, cap, None)
        if patch is not None:
            launch(patch.listed.at(packed), None, patch)
        return patch is not None

    def residual_site(self, site: int, h: torch.Tensor, packed: bool = False) -> bool:
        """Site ``site`` of the residual stream ``h`` (the top of layer ``site``; n_layers: after the last layer):
        ``capture[:, site]`` receives the deciding row of every sequence, and a patch at this site rewrites those of its listed
        sequences (``_capture_and_patch``).  True when rows of ``h`` were rewritten."""
        return self._capture_and_patch(
            None if self.capture is None else self.capture[:, site],
            self.patch if self.patch is not None and self.patch.site == site else None, packed, h.device,
            lambda rows, cap, pt: B.resid_rows(h, rows, capture=cap, **({} if pt is None else pt.operands())))

    def keys_appended(self, layer: int, q: torch.Tensor, kc: torch.Tensor, cfg, max_len: int, packed: bool = False) -> None:
        """q is rotated and the layer's k is in the bf16 cache ``kc``: the readout of the deciding rows' attention, and then —
        the cache holds every prompt position here — of all rows' (``flow``)."""
        if self.readout is not None:
            self.readout.launch(layer, q, self._last if packed else None, kc, cfg, max_len)
            if self.readout.flow is not None:
                assert packed, "the flow readout reads every packed query row: its prefill does not trim the last layer"
                self.readout.launch_flow(layer, q, kc, cfg, max_len)

    def attention_written(self, layer: int, q: torch.Tensor, att: torch.Tensor, kc, vc, cfg, max_len: int,
                          lens: Optional[torch.Tensor] = None, packed: bool = False) -> None:
        """The layer's attention output is in ``att``: a knockout that covers the layer rewrites the listed deciding rows under
        their masks, then cuts that cover it their listed rows.  ``lens``: int32 [n_seqs] key counts (a decode step's; None in a
        prefill: the prompt lengths).  Then the head outputs, as o_proj is about to read them: ``head_capture[:, layer]``
        receives the deciding row of every sequence, and a head patch with a selected head in this layer rewrites those heads
        in the rows of its listed sequences (``_capture_and_patch``).  A layer with neither launches nothing."""
        ko, ct = self.knockout, self.cuts
        if ko is not None and ko.covers(layer):
            ko.launch(q, att, ko.listed.at(packed), kc, vc, self._key_counts if lens is None else lens, cfg, max_len)
        if ct is not None and ct.covers(layer):
            if lens is not None:         # a decode step: the generated rows of the listed sequences under K(generated)
                ct.step.launch(q, att, ct.step.listed.dev, kc, vc, lens, cfg, max_len)
            else:
                ct.launch(self._cut_tables(layer == ct.n_layers - 1, packed, att.device), q, att, kc, vc, cfg, max_len)
        self._capture_and_patch(
            None if self.head_capture is None else self.head_capture[:, layer].flatten(1),
            self.head_patch if self.head_patch is not None and self.head_patch.pairs(layer) is not None else None, packed, att.device,
            lambda rows, cap, hp: B.head_rows(att, rows, n_heads=cfg.n_heads, head_dim=cfg.head_dim, capture=cap,
                                              **({} if hp is None else hp.operands(layer))))

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
# Host side, shared: checks of the caller's arguments (ValueError before any launch) and buffers filled from them
# ================================================================================================
def _need_bf16_kv(what: str, kv_dtype: str) -> None:
    if kv_dtype != "bf16":
        raise ValueError(f"{what} needs the bf16 KV cache (llm_kv_dtype={kv_dtype!r}: the FP8 prefill attends to unrounded "
                         "k / v, so the cache does not hold the keys the attention saw)")


# what a probe that lists something needs and excludes: (the bf16 KV cache, "run(s)", the probes it does not go with — of those
# validated before it — and the refusal's text)
_RUNS = {
    "knockout": (True, "runs", (), None),
    "patch": (False, "runs", ("knockout",), "patch together with knockout is not supported"),
    "head_patch": (False, "runs", ("knockout", "patch"), "head_patch together with knockout or with patch is not supported"),
    "cuts": (True, "run", ("knockout", "patch", "head_patch"), "cuts together with knockout, patch or head_patch is not supported"),
    "want_heads": (False, "runs", (), None),
    "want_hidden": (False, "runs", (), None),
}


def _check_runs(what: str, kv_dtype: str, num_beams: int, others: dict) -> None:
    """The refusals of a probe that is there: the FP8 KV cache, beams, a probe it does not go with (``_RUNS``)."""
    bf16, verb, excluded, text = _RUNS[what]
    if bf16:
        _need_bf16_kv(what, kv_dtype)
    if num_beams != 1:
        raise ValueError(f"{what} {verb} with greedy, sampled and label-constrained decoding, not with beams (num_beams > 1)")
    if any(others.get(o) is not None for o in excluded):
        raise ValueError(text)


def _check_keys(d, what: str, keys: Tuple[str, ...], n_required: int) -> None:
    """``d`` is a dict with the first ``n_required`` of ``keys``, and of the others at most."""
    if not isinstance(d, dict):
        raise ValueError(f"{what} must be a dict with the keys {keys}")
    unknown = set(d) - set(keys)
    if unknown or any(k not in d for k in keys[:n_required]):
        optional = [repr(k) for k in keys[n_required:]]
        raise ValueError(f"{what} holds {' and '.join(repr(k) for k in keys[:n_required])}, and optionally {', '.join(optional[:-1])} and "
                         f"{optional[-1]} (unknown keys: {sorted(unknown)})")


def _check_segments(prefix: str, segments, plens: List[int], note: str) -> List[np.ndarray]:
    """One list of segment ids 0..255 per prompt, one id per position, as int64 arrays."""
    if len(segments) != len(plens):
        raise ValueError(f"{prefix}{len(segments)} segment lists for {len(plens)} prompts")
    segs = []
    for b, (sg, n) in enumerate(zip(segments, plens)):
        try:
            sg = np.asarray(sg.cpu() if isinstance(sg, torch.Tensor) else sg).astype(np.int64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{prefix}segments[{b}] must be a list of segment ids") from None
        if len(sg) != n:
            raise ValueError(f"{prefix}segments[{b}] has {len(sg)} entries, the prompt of row {b} has {n} positions")
        if len(sg) and (sg.min() < 0 or sg.max() > 255):
            raise ValueError(f"{prefix}segments[{b}]: segment ids are 0..255 ({note})")
        segs.append(sg)
    return segs


def _check_window(what: str, layers, heads, cfg):
    """((l0, l1), heads): a non-empty half-open range of decoder layers (None: all) and None (all) or a sorted tuple of query heads."""
    if layers is None:
        layers = (0, cfg.n_layers)
    try:
        l0, l1 = (int(x) for x in layers)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: layers must be a half-open range (l0, l1), not {layers!r}") from None
    if not 0 <= l0 < l1 <= cfg.n_layers:
        raise ValueError(f"{what}: layer window ({l0}, {l1}) must be a non-empty range inside [0, {cfg.n_layers}]")
    if heads is not None:
        try:
            heads = tuple(sorted({int(x) for x in heads}))
        except (TypeError, ValueError):
            raise ValueError(f"{what}: heads must be None or a list of query-head indices, not {heads!r}") from None
        if not heads or heads[0] < 0 or heads[-1] >= cfg.n_heads:
            raise ValueError(f"{what}: head indices {list(heads)} must be a non-empty subset of 0..{cfg.n_heads - 1}")
    return (l0, l1), heads


def _segment_table(ws: Workspace, name: str, segs, max_len: int) -> torch.Tensor:
    """uint8 [n_seqs, max_len] in workspace buffer ``name``: the segment of every cache position, ``IGNORE_SEGMENT`` past the prompt."""
    seg = torch.full((len(segs), max_len), IGNORE_SEGMENT, dtype=torch.uint8)
    for b, sg in enumerate(segs):
        seg[b, :len(sg)] = torch.as_tensor(sg, dtype=torch.uint8)
    seg_d = ws.get(name, tuple(seg.shape), torch.uint8)
    seg_d.copy_(seg, non_blocking=True)
    return seg_d


def _masked_rows(ws: Workspace, prefix: str, cfg, seg_d: torch.Tensor, masks: List[int], head_on: np.ndarray, layers) -> Knockout:
    """The operands of icl_attn_decode_masked_bf16 in the workspace buffers ``prefix``_blocked and ``prefix``_rows: the sequences
    with a non-zero u32 bit set in ``masks`` and, per (listed sequence, query head), that set where the head is on, else 0."""
    listed = [b for b, m in enumerate(masks) if m]
    bits = np.where(head_on[None, :], _as_i32_bits([masks[b] for b in listed])[:, None], 0).astype(np.int32)
    blk_d = ws.get(prefix + "_blocked", bits.shape, I32)
    rows_d = ws.get(prefix + "_rows", (len(listed),), I32)
    blk_d.copy_(torch.from_numpy(bits), non_blocking=True)
    return Knockout(seg_d, blk_d, RowList.filled(rows_d, listed), layers)


def _heads_on(cfg, heads) -> np.ndarray:
    """bool [n_heads]: the query heads a head subset switches on (None: all)."""
    on = np.zeros(cfg.n_heads, dtype=bool)
    on[list(range(cfg.n_heads) if heads is None else heads)] = True
    return on


def _rows_of(vec: torch.Tensor, rows: List[int]) -> torch.Tensor:
    """Per-prompt vectors of the prompts ``rows``; shared vectors (one leading entry) as they are."""
    return vec if vec.shape[0] == 1 else vec[torch.tensor(rows, device=vec.device)]


# ================================================================================================
# The readout (``prompt_attention``)
# ================================================================================================
def check_readout(segments, n_seg: Optional[int], kv_dtype: str, plens: List[int]) -> Tuple[List[torch.Tensor], int]:
    """Host validation of ``prompt_attention(segments=, n_seg=)``: (segments as int64 tensors, the segment count)."""
    _need_bf16_kv("prompt_attention", kv_dtype)
    segs = [torch.from_numpy(sg) for sg in _check_segments("", segments, plens, f"{IGNORE_SEGMENT} = counted nowhere")]
    if n_seg is None:
        n_seg = 1 + max(int(sg[sg < IGNORE_SEGMENT].max()) if bool((sg < IGNORE_SEGMENT).any()) else 0 for sg in segs)
    if not 1 <= int(n_seg) <= MAX_READOUT_SEGMENTS:
        raise ValueError(f"{n_seg} segments: the readout kernel sums at most {MAX_READOUT_SEGMENTS}")
    return segs, int(n_seg)


def readout_state(ws: Workspace, cfg, segs: List[torch.Tensor], n_seg: int, lens: List[int], max_len: int, want_probs: bool,
                  device, want_flow: bool = False) -> AttnReadout:
    """The validated readout on the device: the segment table padded to the cache length, the prompt lengths, and where the
    launches leave the mass (and the full weights, ``want_probs``: zeroed — the kernel leaves a row's tail untouched; and the
    segment-to-segment flow, ``want_flow``: every element is written)."""
    Bn = len(segs)
    seg_d = _segment_table(ws, "pa_seg", segs, max_len)
    mass = ws.get("pa_mass", (cfg.n_layers, Bn, cfg.n_heads, n_seg), F32)
    probs = ws.get("pa_probs", (cfg.n_layers, Bn, cfg.n_heads, max_len), F32) if want_probs else None
    if probs is not None:
        probs.zero_()
    flow = ws.get("pa_flow", (cfg.n_layers, Bn, cfg.n_heads, n_seg, n_seg), F32) if want_flow else None
    return AttnReadout(seg_d, _i32(lens, device), mass, probs, flow)


# ================================================================================================
# The probe arguments of ``generate``: each check returns a dict that is itself a valid argument, or None when the probe lists
# nothing — the call is then the plain one.  ``runs()`` raises the refusals of a probe that is there (``_check_runs``), at the
# point of each check where they have always been raised
# ================================================================================================
def _check_knockout(knockout, cfg, plens: List[int], runs):
    """``generate(knockout=...)``: ``segments`` as int64 arrays, ``blocked`` as sorted tuples, ``layers`` (l0, l1), ``heads`` a
    tuple or None; None when every set is empty."""
    if isinstance(knockout, dict):
        _check_keys(knockout, "knockout", KNOCKOUT_KEYS, 2)
        knockout = tuple(knockout.get(k) for k in KNOCKOUT_KEYS)
    try:
        segments, blocked, layers, heads = (tuple(knockout) + (None, None))[:4] if 2 <= len(knockout) <= 4 else (None,) * 4
    except TypeError:
        segments = None
    if segments is None:
        raise ValueError("knockout must be (segments, blocked[, layers[, heads]]) or a dict with those keys")
    if len(segments) != len(plens) or len(blocked) != len(plens):
        raise ValueError(f"knockout: {len(segments)} segment lists and {len(blocked)} blocked sets for {len(plens)} prompts")
    segs = _check_segments("knockout: ", segments, plens, f"ids >= {MAX_KNOCKOUT_SEGMENTS} are never blocked")
    sets = []
    for b, given in enumerate(blocked):
        bl = tuple(sorted({int(x) for x in given}))
        if bl and not (0 <= bl[0] and bl[-1] < MAX_KNOCKOUT_SEGMENTS):
            raise ValueError(f"knockout: blocked[{b}] = {list(bl)}: only segment ids 0..{MAX_KNOCKOUT_SEGMENTS - 1} can be blocked")
        sets.append(bl)
    layers, heads = _check_window("knockout", layers, heads, cfg)
    for b, (sg, bl) in enumerate(zip(segs, sets)):
        if bl and bool(np.isin(sg, bl).all()):
            raise ValueError(f"knockout: row {b}: the blocked segments {list(bl)} cover every position of its prompt")
    if not any(sets):
        return None
    runs()
    return dict(segments=segs, blocked=sets, layers=layers, heads=heads)


def _knockout_state(ws: Workspace, cfg, knockout, max_len: int) -> Knockout:
    """The validated knockout on the device, in graph-visible workspace buffers refilled on every call: the segment table
    padded to the cache length, the listed rows (non-empty sets) and their per-head bit sets."""
    seg_d = _segment_table(ws, "gen_ko_seg", knockout["segments"], max_len)
    return _masked_rows(ws, "gen_ko", cfg, seg_d, [sum(1 << g for g in bl) for bl in knockout["blocked"]],
                        _heads_on(cfg, knockout["heads"]), knockout["layers"])


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


def _check_cuts(cuts, cfg, plens: List[int], runs):
    """``generate(cuts=...)``: the arguments in one form (``segments`` as int64 arrays, ``pairs`` one list per prompt,
    ``generated`` one id per prompt, ``layers`` (l0, l1), ``heads`` a tuple or None: the ``CUT_KEYS``, themselves valid ``cuts``)
    and what follows from them: ``entries[b]`` the listed positions of prompt b and their bit sets K(seg[p]), two int64 arrays,
    ``gen[b]`` the bit set of prompt b's generated rows (0: untouched) — or None when no row is listed and no generated row cuts
    anything.

    Position p of prompt b is listed iff at least one key j <= p has seg[j] in K(seg[p])."""
    _check_keys(cuts, "cuts", CUT_KEYS, 2)
    n = len(plens)
    segs = _check_segments("cuts: ", cuts["segments"], plens, f"ids >= {MAX_CUT_SEGMENTS} are never cut")
    Ks = _cut_pairs(cuts["pairs"], n)
    layers, heads = _check_window("cuts", cuts.get("layers"), cuts.get("heads"), cfg)
    generated = cuts.get("generated")
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
    runs()
    pairs = [[(a, g) for a, m in sorted(K.items()) for g in range(MAX_CUT_SEGMENTS) if (m >> g) & 1] for K in Ks]
    return dict(segments=segs, pairs=pairs, generated=gen_ids, entries=tuple(entries), gen=gen, layers=layers, heads=heads)


def _cuts_state(ws: Workspace, cfg, cuts, max_len: int) -> Cuts:
    """The validated cuts: the per-sequence host lists of listed positions and bit sets, and on the device, in graph-visible
    workspace buffers refilled on every call, the segment table padded to the cache length, the head switch, and the decode
    steps' state for the sequences whose generated rows cut something (a ``Knockout`` over the same segment table)."""
    seg_d = _segment_table(ws, "gen_ct_seg", cuts["segments"], max_len)
    on, head_on = _heads_on(cfg, cuts["heads"]), None
    if not on.all():
        head_on = ws.get("gen_ct_heads", (cfg.n_heads,), torch.uint8)
        head_on.copy_(torch.from_numpy(on.astype(np.uint8)), non_blocking=True)
    R = B.load_library().icl_attn_cut_tile_rows(cfg.n_heads, cfg.kv_heads, cfg.head_dim)      # a host query of the library, no launch
    if R <= 0:
        raise ValueError(f"cuts: no row-tile attention form for n_heads={cfg.n_heads}, n_kv_heads={cfg.kv_heads}, head_dim={cfg.head_dim}")
    step = _masked_rows(ws, "gen_ct", cfg, seg_d, cuts["gen"], on, cuts["layers"]) if any(cuts["gen"]) else None
    return Cuts(seg_d, cuts["entries"], cuts["layers"], cfg.n_layers, R, head_on, step)


def _check_rows_patch(d: dict, what: str, where: dict, inner: Tuple[int, ...], per: str, order: str, n_prompts: int, runs):
    """What ``patch`` and ``head_patch`` share: ``vectors`` f32 [n_prompts or 1, *inner] (or [*inner]: shared), ``mode``,
    ``steps``, ``alpha`` and ``rows``.  Returns ``where`` plus these, ``vectors`` with its leading dimension and ``rows`` an
    ascending list (all prompts for None), or None when ``rows`` is empty."""
    vec, dims = d["vectors"], ", ".join(str(x) for x in inner)
    if not isinstance(vec, torch.Tensor) or vec.dtype != F32:
        raise ValueError(f"{what}: vectors must be a float32 tensor")
    if vec.dim() == len(inner):
        vec = vec[None]
    if vec.dim() != len(inner) + 1 or tuple(vec.shape[1:]) != inner or vec.shape[0] not in (1, n_prompts):
        raise ValueError(f"{what}: vectors of shape {tuple(d['vectors'].shape)}: [{n_prompts}, {dims}] ({per} per prompt), [1, {dims}] "
                         f"or [{dims}] (shared){order}")
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
    runs()
    return dict(where, vectors=vec, mode=mode, alpha=alpha, rows=rows, steps=steps) if rows else None


def _check_patch(patch, cfg, plens: List[int], runs):
    """``generate(patch=...)``: the patch as a dict of all ``PATCH_KEYS`` — ``vectors`` f32 [n_prompts or 1, hidden]."""
    _check_keys(patch, "patch", PATCH_KEYS, 2)
    site = patch["site"]
    if isinstance(site, bool) or not isinstance(site, int) or not 0 <= site <= cfg.n_layers:
        raise ValueError(f"patch: site {site!r} must be an integer in 0..{cfg.n_layers} (n_layers = the last layer's output)")
    return _check_rows_patch(patch, "patch", dict(site=site), (cfg.hidden,), "one", "", len(plens), runs)


def _check_head_patch(hp, cfg, plens: List[int], runs):
    """``generate(head_patch=...)``: the patch as a dict of all ``HEAD_PATCH_KEYS`` — ``heads`` a list of (layer, head) as given,
    ``vectors`` f32 [n_prompts or 1, n_pairs, head_dim] in that order."""
    _check_keys(hp, "head_patch", HEAD_PATCH_KEYS, 2)
    pairs = check_head_pairs(hp["heads"], cfg, "head_patch")
    return _check_rows_patch(hp, "head_patch", dict(heads=pairs), (len(pairs), cfg.head_dim), "one block", ", in the order of heads",
                             len(plens), runs)


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


def _patch_state(ws: Workspace, cfg, patch) -> ResidPatch:
    """The validated patch on the device, in graph-visible workspace buffers refilled on every call: the listed rows'
    vectors (one row of the buffer when the vector is shared) and the listed sequences."""
    vec, rows = _rows_of(patch["vectors"], patch["rows"]), patch["rows"]
    vec_d = ws.get("gen_rp_vec", (vec.shape[0], cfg.hidden), F32)
    rows_d = ws.get("gen_rp_rows", (len(rows),), I32)
    vec_d.copy_(vec, non_blocking=True)
    return ResidPatch(vec_d, RowList.filled(rows_d, rows), patch["mode"], patch["alpha"], patch["steps"], patch["site"])


def _head_patch_state(ws: Workspace, cfg, hp) -> HeadPatch:
    """The validated head patch on the device, in graph-visible workspace buffers refilled on every call: the head indices
    sorted by (layer, head), the listed rows' vectors permuted to that order (one block when they are shared) and the listed
    sequences."""
    pairs, rows = hp["heads"], hp["rows"]
    order = sorted(range(len(pairs)), key=lambda i: pairs[i])
    vec = _rows_of(hp["vectors"][:, torch.tensor(order, device=hp["vectors"].device)], rows)
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
    return HeadPatch(vec_d, RowList.filled(rows_d, rows), hp["mode"], hp["alpha"], hp["steps"], heads_d, tuple(layers))


@dataclass
class ProbeArgs:
    """The validated probe arguments of one ``generate`` call, under the names ``generate`` takes them (``vars()`` of it are
    keyword arguments that validate to the same): each probe a dict, or None — not given, or it lists nothing."""
    knockout: Optional[dict] = None
    patch: Optional[dict] = None
    head_patch: Optional[dict] = None
    cuts: Optional[dict] = None
    want_hidden: bool = False
    want_heads: bool = False

    def kept(self, keep: List[int]) -> "ProbeArgs":
        """``overlong="drop"``: the arguments of the call over the prompts ``keep`` — the surviving rows' entries and vectors, a
        patch's rows under the indices they have among the survivors."""
        pick = lambda d, *per_prompt: dict(d, **{k: [d[k][b] for b in keep] for k in per_prompt})
        patched = lambda d: dict(d, vectors=_rows_of(d["vectors"], keep), rows=[keep.index(b) for b in d["rows"] if b in keep])
        ko, pt, hp, ct = self.knockout, self.patch, self.head_patch, self.cuts
        return replace(self, knockout=ko and pick(ko, "segments", "blocked"), patch=pt and patched(pt), head_patch=hp and patched(hp),
                       cuts=ct and pick({k: ct[k] for k in CUT_KEYS}, "segments", "pairs", "generated"))

    def state(self, ws: Workspace, cfg, n_seqs: int, max_len: int) -> Probes:
        """The bundle of the call on the device, in graph-visible workspace buffers refilled on every call (a plain call
        requests none): where the captures go, and the state of every probe that is there."""
        hidden = ws.get("gen_hidden", (n_seqs, cfg.n_layers + 1, cfg.hidden), F32) if self.want_hidden else None
        head_out = ws.get("gen_head_out", (n_seqs, cfg.n_layers, cfg.n_heads, cfg.head_dim), BF16) if self.want_heads else None
        return Probes(knockout=self.knockout and _knockout_state(ws, cfg, self.knockout, max_len), capture=hidden,
                      patch=self.patch and _patch_state(ws, cfg, self.patch),
                      head_capture=head_out, head_patch=self.head_patch and _head_patch_state(ws, cfg, self.head_patch),
                      cuts=self.cuts and _cuts_state(ws, cfg, self.cuts, max_len))


def check_probes(cfg, kv_dtype: str, plens: List[int], num_beams: int, knockout=None, patch=None, head_patch=None, cuts=None,
                 want_hidden: bool = False, want_heads: bool = False) -> ProbeArgs:
    """Host validation of the probe arguments of ``generate``, as the caller gave them: everything is a ``ValueError`` raised
    before any launch.  A probe that lists nothing — every blocked set empty, an empty row list, cuts no query meets — is None
    in the result and refuses nothing: the call is then the plain one, beams included."""
    got = dict(knockout=None, patch=None, head_patch=None, cuts=None)
    runs = lambda what: _check_runs(what, kv_dtype, num_beams, got)
    for name, given, check in (("knockout", knockout, _check_knockout), ("patch", patch, _check_patch),
                               ("head_patch", head_patch, _check_head_patch), ("cuts", cuts, _check_cuts)):
        if given is not None:
            got[name] = check(given, cfg, plens, lambda name=name: runs(name))
    if want_heads:
        runs("want_heads")
    if want_hidden:
        runs("want_hidden")
    return ProbeArgs(want_hidden=bool(want_hidden), want_heads=bool(want_heads), **got)
