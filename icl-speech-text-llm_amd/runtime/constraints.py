"""Label automata for constrained greedy decoding (opt-in; ``generate(..., constraint=...)``, batch key ``constrain_labels``).

A closed-set task (``data/task_prompts.json``: ``valid_labels``) has a small language of valid completions — ONE label, or a
``", "``-joined list of labels — in the strings ``data/multi_task_dataset._format_label`` writes.  ``build_label_automaton`` turns
that language, as the model's own tokenizer cuts it, into a deterministic token automaton in CSR form; the decode tail
``icl_argmax_fsm`` (include/icl_hip.h) then picks every token among the outgoing edges of the row's state instead of the whole
vocabulary, so the decoded text is a valid answer by construction and needs no repair by ``clean_prediction``.

Everything here is host code (pure Python + torch CPU tensors) and imports without a GPU; ``LabelAutomaton.upload`` is the one
place that touches a device.
"""
from __future__ import annotations

import itertools
import logging
import re
from collections import deque
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from ..data.task_configs import DatasetType, get_dataset_config, is_swap_type

logger = logging.getLogger(__name__)

FREE = -1                                        # start state of a row that is decoded without a constraint
SINGLE_LABEL_TYPES = ("VOXCELEB", "VOXCELEB_GREEK", "MELD", "MELD_GREEK", "MELD_EMOTION", "MELD_EMOTION_GREEK")
LIST_TYPES = ("HVB", "HVB_GREEK", "VOXPOPULI", "VOXPOPULI_GREEK")
NONE_TYPES = ("VOXPOPULI", "VOXPOPULI_GREEK")    # an empty list is written "none"

_upload_ids = itertools.count(1)
_logged_free = set()


class DeviceTables:
    """One upload of an automaton's tables; ``uid`` identifies the upload (captured decode graphs are keyed by it)."""

    def __init__(self, a: "LabelAutomaton", device):
        self.state_off, self.edge_tok = a.state_off.to(device), a.edge_tok.to(device)
        self.edge_next, self.state_dist = a.edge_next.to(device), a.state_dist.to(device)
        self.n_states, self.n_edges, self.vocab = a.n_states, a.n_edges, a.vocab
        self.uid = next(_upload_ids)


class LabelAutomaton:
    """Deterministic token automaton in CSR form.

    ``state_off`` int32 [S+1], ``edge_tok`` / ``edge_next`` int32 [E]: the edges of state s are ``state_off[s] .. state_off[s+1]-1``,
    sorted by token id and unique.  A state is *accepting* when it has an edge on ``eos_id`` (which must lead back to it).
    ``state_dist`` int32 [S] = the fewest tokens from a state to an accepting one (0 for an accepting state), computed here.
    ``starts``: grammar name (a dataset type's value) -> start state, ``FREE`` for a type without a grammar.
    The constructor validates everything a kernel later trusts and raises ``ValueError`` otherwise."""

    def __init__(self, state_off, edge_tok, edge_next, starts: Dict[str, int], vocab: int, eos_id: int):
        off = [int(x) for x in state_off]
        tok = [int(x) for x in edge_tok]
        nxt = [int(x) for x in edge_next]
        S, E, V = len(off) - 1, len(tok), int(vocab)
        if S < 1 or E < 1 or V < 1:
            raise ValueError(f"empty automaton: {S} states, {E} edges, vocabulary {V}")
        if len(nxt) != E or off[0] != 0 or off[-1] != E or any(off[s] > off[s + 1] for s in range(S)):
            raise ValueError("state_off must rise from 0 to the number of edges, edge_tok and edge_next must have one entry per edge")
        if not 0 <= int(eos_id) < V:
            raise ValueError(f"EOS id {eos_id} outside the vocabulary [0,{V})")
        for s in range(S):
            row = tok[off[s]:off[s + 1]]
            if any(not 0 <= t < V for t in row):
                raise ValueError(f"state {s}: token id outside the vocabulary [0,{V})")
            if any(row[i] >= row[i + 1] for i in range(len(row) - 1)):
                raise ValueError(f"state {s}: edges must be sorted by token id and unique")
            for e in range(off[s], off[s + 1]):
                if not 0 <= nxt[e] < S:
                    raise ValueError(f"state {s}: next state {nxt[e]} outside [0,{S})")
                if tok[e] == eos_id and nxt[e] != s:
                    raise ValueError(f"state {s}: the EOS edge of an accepting state must lead back to it")
        for name, st in starts.items():
            if not -1 <= int(st) < S:
                raise ValueError(f"start state {st} of {name!r} outside [-1,{S})")
        # fewest tokens to an accepting state: breadth-first search over the reversed edges
        rev: List[List[int]] = [[] for _ in range(S)]
        dist = [-1] * S
        queue = deque()
        for s in range(S):
            for e in range(off[s], off[s + 1]):
                if tok[e] == eos_id:
                    dist[s] = 0
                    queue.append(s)
                else:
                    rev[nxt[e]].append(s)
        while queue:
            s = queue.popleft()
            for p in rev[s]:
                if dist[p] < 0:
                    dist[p] = dist[s] + 1
                    queue.append(p)
        dead = [s for s in range(S) if dist[s] < 0]
        if dead:
            raise ValueError(f"state(s) {dead[:8]} cannot reach an accepting state")
        i32 = torch.int32
        self.state_off, self.edge_tok = torch.tensor(off, dtype=i32), torch.tensor(tok, dtype=i32)
        self.edge_next, self.state_dist = torch.tensor(nxt, dtype=i32), torch.tensor(dist, dtype=i32)
        self.n_states, self.n_edges, self.vocab, self.eos_id = S, E, V, int(eos_id)
        self.starts = {str(k): int(v) for k, v in starts.items()}
        self._off, self._tok, self._nxt, self._dist = off, tok, nxt, dist
        self._device: Dict[str, DeviceTables] = {}

    # ---- host-side walking (validation, tests, the CLI's checks) -----------------------------------------------------------
    def edges(self, state: int) -> List[Tuple[int, int]]:
        return [(self._tok[e], self._nxt[e]) for e in range(self._off[state], self._off[state + 1])]

    def is_accepting(self, state: int) -> bool:
        return self._dist[state] == 0

    def min_tokens(self, state: int) -> int:
        return 0 if state < 0 else self._dist[state]

    def candidates(self, state: int, steps_left: int) -> List[Tuple[int, int]]:
        """The (token, next state) pairs the budget rule leaves at ``state`` with ``steps_left`` tokens to go, this one included."""
        return [(t, n) for t, n in self.edges(state) if self._dist[n] <= steps_left - 1]

    def walk(self, start: int, ids: Iterable[int]) -> int:
        """State after ``ids`` from ``start``; -2 when a token has no edge.  Tokens after an EOS are ignored (pad fill)."""
        s = start
        for t in ids:
            t = int(t)
            step = dict(self.edges(s)).get(t)
            if step is None:
                return -2
            s = step
            if t == self.eos_id:
                break
        return s

    def accepts(self, start: int, ids: Iterable[int]) -> bool:
        s = self.walk(start, ids)
        return s >= 0 and self.is_accepting(s)

    def start_states(self, dataset_types: Sequence) -> List[int]:
        out = []
        for dt in dataset_types:
            key = DatasetType(dt).value
            if key not in self.starts:
                raise ValueError(f"no grammar for dataset type {key!r} in this automaton (built for {sorted(self.starts)})")
            out.append(self.starts[key])
        return out

    def upload(self, device) -> DeviceTables:
        """The tables on ``device`` (uploaded once per device and kept)."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = DeviceTables(self, device)
        return self._device[key]


# ---------------------------------------------------------------------------------------------------------------------
# grammars
# ---------------------------------------------------------------------------------------------------------------------
def grammar_of(dataset_type) -> Tuple[str, List[str]]:
    """("free" | "single" | "list" | "list+none", lower-cased labels) of a dataset type."""
    dt = DatasetType(dataset_type)
    cfg = get_dataset_config(dt)
    labels = getattr(cfg, "valid_labels", None)
    if not labels or is_swap_type(dt):             # no closed set, or a swap type whose mapping is drawn per item
        return "free", []
    labels = [str(l).lower() for l in labels]
    if dt.name in SINGLE_LABEL_TYPES:
        return "single", labels
    if dt.name in LIST_TYPES:
        return ("list+none" if dt.name in NONE_TYPES else "list"), labels
    return "free", []


def _ids(tokenizer, text: str) -> List[int]:
    """Token ids of a completion, as ``CustomSALMONN.forward`` tokenises one."""
    enc = tokenizer(text, add_special_tokens=False)["input_ids"]
    return [int(t) for t in (enc.reshape(-1).tolist() if hasattr(enc, "reshape") else enc)]


def _norm_ws(s: str) -> str:
    return re.sub(r"\s+", " ", s).strip()


def _check_decode(tokenizer, text: str, ids: List[int]) -> None:
    back = tokenizer.decode(ids, skip_special_tokens=True)
    if _norm_ws(back) != _norm_ws(text):
        raise ValueError(f"the tokenizer does not decode {text!r} back from its own ids (got {back!r}): no automaton for it")


def _common_prefix(seqs: List[List[int]]) -> List[int]:
    n = 0
    while all(len(s) > n for s in seqs) and len({s[n] for s in seqs}) == 1:
        n += 1
    return seqs[0][:n]


class _Trie:
    """States of one grammar: node 0 = start, node 1 = "next label" (lists only)."""

    def __init__(self):
        self.children: List[Dict[int, int]] = [{}]
        self.accepting = {0: False}
        self.redirect: Dict[int, int] = {}        # node -> the "next label" node it stands for

    def node(self) -> int:
        self.children.append({})
        self.accepting[len(self.children) - 1] = False
        return len(self.children) - 1

    def add(self, root: int, ids: List[int], what: str) -> int:
        if not ids:
            raise ValueError(f"{what}: empty token sequence")
        s = root
        for t in ids:
            if t not in self.children[s]:
                self.children[s][t] = self.node()
            s = self.children[s][t]
        return s


def _single_paths(tokenizer, labels: List[str], trie: _Trie) -> None:
    for a in labels:
        ids = _ids(tokenizer, a)
        _check_decode(tokenizer, a, ids)
        trie.accepting[trie.add(0, ids, a)] = True


def _list_paths(tokenizer, labels: List[str], with_none: bool, trie: _Trie) -> None:
    """F / H / M / T tables of the tokenizer over this label set, verified on every list of one, two and three labels."""
    sep = ", "
    if len(labels) < 2:
        raise ValueError("a label-list grammar needs at least two labels")
    F = {a: _ids(tokenizer, a) for a in labels}
    pair = {(a, b): _ids(tokenizer, a + sep + b) for a in labels for b in labels}
    H = {a: _common_prefix([pair[a, b] for b in labels]) for a in labels}
    a0 = labels[0]
    T = {b: pair[a0, b][len(H[a0]):] for b in labels}
    for (a, b), ids in pair.items():
        if ids != H[a] + T[b]:
            raise ValueError(f"the tokenizer cuts {a + sep + b!r} in a way that depends on the neighbouring label: no automaton for it")
    M: Dict[str, List[int]] = {}
    c0 = labels[0]
    for b in labels:
        ids = _ids(tokenizer, a0 + sep + b + sep + c0)
        h, t = H[a0], T[c0]
        if ids[:len(h)] != h or len(ids) < len(h) + len(t) or ids[len(ids) - len(t):] != t:
            raise ValueError(f"the tokenizer cuts {a0 + sep + b + sep + c0!r} in a way that depends on the neighbouring label")
        M[b] = ids[len(h):len(ids) - len(t)]
    for a in labels:
        _check_decode(tokenizer, a, F[a])
        for b in labels:
            _check_decode(tokenizer, a + sep + b, pair[a, b])
            for c in labels:
                text = a + sep + b + sep + c
                ids = _ids(tokenizer, text)
                if ids != H[a] + M[b] + T[c]:
                    raise ValueError(f"the tokenizer cuts {text!r} in a way that depends on the neighbouring labels: no automaton for it")
                _check_decode(tokenizer, text, ids)
    nxt = trie.node()                              # the "next label" state
    ends_next = []
    for a in labels:
        trie.accepting[trie.add(0, F[a], a)] = True
    for a in labels:
        ends_next.append((trie.add(0, H[a], a + sep), a + sep))
    for b in labels:
        trie.accepting[trie.add(nxt, T[b], sep + b)] = True
    for b in labels:
        ends_next.append((trie.add(nxt, M[b], sep + b + sep), sep + b + sep))
    if with_none:
        if "none" in labels:
            raise ValueError("'none' is both a label and the empty list")
        ids = _ids(tokenizer, "none")
        _check_decode(tokenizer, "none", ids)
        trie.accepting[trie.add(0, ids, "none")] = True
    # the end of an H / M path IS the "next label" state: it may carry nothing of its own, or the automaton would have to guess
    for node, what in ends_next:
        if trie.children[node] or trie.accepting[node] or node in (0, nxt):
            raise ValueError(f"the token path of {what!r} is a prefix of (or equal to) another path: no deterministic automaton for it")
        trie.redirect[node] = nxt


def _emit(trie: _Trie, eos_id: int, base: int):
    """CSR rows of one grammar with state ids offset by ``base``; redirected nodes are dropped and renumbered away."""
    keep = [n for n in range(len(trie.children)) if n not in trie.redirect]
    new_id = {n: base + i for i, n in enumerate(keep)}
    for n, target in trie.redirect.items():
        new_id[n] = new_id[target]
    rows = []
    for n in keep:
        edges = {t: new_id[c] for t, c in trie.children[n].items()}
        if trie.accepting[n]:
            if eos_id in edges:
                raise ValueError("a label's token path uses the EOS id")
            edges[eos_id] = new_id[n]
        if not edges:
            raise ValueError("a state without edges: a path ends without being accepted")
        rows.append(sorted(edges.items()))
    return rows


def build_label_automaton(tokenizer, dataset_types: Sequence, eos_id: Optional[int] = None,
                          vocab: Optional[int] = None) -> LabelAutomaton:
    """One automaton over the grammars of ``dataset_types`` (state ids of each grammar offset, so a mixed batch is one launch).

    Single-label types: ``label EOS``.  HVB / VoxPopuli (and ``_greek``): ``label (", " label)* EOS`` — repeating a label is
    allowed — plus ``none EOS`` for VoxPopuli.  Types without a closed label set and swap types are *free* (start state -1).
    The token paths come from ``tokenizer`` itself and are verified on every list of up to three labels; a tokenizer whose cut
    of a label depends on its neighbours, or that does not decode its own ids back to the text, gets a ``ValueError`` naming the
    string.  ``vocab`` defaults to ``len(tokenizer)``, ``eos_id`` to ``tokenizer.eos_token_id``."""
    eos_id = int(tokenizer.eos_token_id if eos_id is None else eos_id)
    vocab = int(len(tokenizer) if vocab is None else vocab)
    rows_all, starts = [], {}
    for dt in dict.fromkeys(DatasetType(d) for d in dataset_types):
        kind, labels = grammar_of(dt)
        if kind == "free":
            starts[dt.value] = FREE
            if dt.value not in _logged_free:
                _logged_free.add(dt.value)
                logger.info("constrained decoding: %s has no closed label set (or draws its mapping per item): decoded freely", dt.value)
            continue
        trie = _Trie()
        if kind == "single":
            _single_paths(tokenizer, labels, trie)
        else:
            _list_paths(tokenizer, labels, kind == "list+none", trie)
        starts[dt.value] = len(rows_all)
        rows_all.extend(_emit(trie, eos_id, len(rows_all)))
    if not rows_all:
        raise ValueError(f"none of {[DatasetType(d).value for d in dataset_types]} has a closed label set: nothing to constrain")
    off, tok, nxt = [0], [], []
    for row in rows_all:
        tok.extend(t for t, _ in row)
        nxt.extend(n for _, n in row)
        off.append(len(tok))
    return LabelAutomaton(off, tok, nxt, starts, vocab, eos_id)


def constraint_for_batch(cache: dict, tokenizer, dataset_types: Sequence, eos_id: int, vocab: int):
    """(automaton, start states) for the rows of one batch, or ``None`` when every row is free; automata are kept in ``cache`` (the
    plugin's), one per set of dataset types."""
    values = [DatasetType(d).value for d in dataset_types]
    key = (tuple(sorted(set(values))), int(eos_id), int(vocab))
    if key not in cache:
        if all(grammar_of(v)[0] == "free" for v in key[0]):
            build = None
            for v in key[0]:
                if v not in _logged_free:
                    _logged_free.add(v)
                    logger.info("constrained decoding: %s has no closed label set (or draws its mapping per item): decoded freely", v)
        else:
            build = build_label_automaton(tokenizer, key[0], eos_id=eos_id, vocab=vocab)
        cache[key] = build
    automaton = cache[key]
    return None if automaton is None else (automaton, automaton.start_states(values))
