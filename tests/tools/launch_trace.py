"""Launch trace of the Llama decoder runtime (runtime/engines.py: LlamaHIP.prefill / decode_step / logits), on the CPU.

What the decoder runtime DOES is the sequence of library launches it makes: the kernels are in libicl_hip, the Python only
chooses which to call, on which operands, in which order.  This tool runs the public methods of ``LlamaHIP`` over a matrix of
model shapes, weight / KV modes, switches and batch sizes with every launching wrapper of ``runtime.binding`` replaced by a
recorder, and reduces what it saw to one sha256 per (config, weight mode, KV dtype, switch) group.  Two versions of
engines.py with the same digests make the same calls with the same operands in the same order — bit-identical results and
the same device time by construction.  tests/test_launch_trace.py compares against tests/golden/llama_launch_trace.json.

A second matrix pins the generation driver one level up (runtime/salmonn.py: ``generate`` with every decode tail, chunked
prefill, ``overlong="drop"`` and beam search, and the probes of the deciding rows — ``prompt_attention``, ``knockout``,
``want_hidden``, ``patch``, ``want_heads``, ``head_patch`` and ``cuts`` — chunked and not): one sha256 per case in tests/golden/generate_launch_trace.json.  Besides the
launches, a generate trace holds the torch plumbing between them (every in-place op or ``clone`` on a device tensor, host
tables by value), where the three ``phase_marks`` are recorded, and the shape of the result.

Nothing is computed: the weights are ``torch.empty`` tensors on the ``meta`` device (real 7B dims cost no memory).  The only
library entry point reached is icl_gemm_select_tile (``binding.rope_fusable``), which needs the built library but no GPU.
The one device-to-host copy at the end of ``generate`` reads zeros (``Tensor.cpu`` of a ``meta`` tensor, inside the tool only).

    python tests/tools/launch_trace.py                 compare with both fixtures, list the groups / cases that differ
    python tests/tools/launch_trace.py --write         regenerate both fixtures
    python tests/tools/launch_trace.py --dump DIR      also write the full text of every case, one file per group / generate case
    python tests/tools/launch_trace.py --root TREE     trace TREE's package instead of this tree's (another checkout of the
                                                       repository; ICL_LIB_PATH names the built library if TREE has none)

A digest that differs is diffed with two ``--dump`` directories, one per tree.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import importlib
import inspect
import json
import os
import sys
from dataclasses import fields, replace

import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(ROOT, "tests", "golden", "llama_launch_trace.json")
GEN_FIXTURE = os.path.join(ROOT, "tests", "golden", "generate_launch_trace.json")

NOT_LAUNCHES = ("load_library", "rope_epilogue_ok", "rope_fusable", "device_cu_count")
RETURNS_OUT = ("gemm", "gemm_rmsnorm", "gather_rows")        # wrappers whose result is their ``out`` operand
N_CU = 256                                                   # MI355X; also the library's answer without a device
CACHE_LEN = 448

WEIGHT_MODES = KV_DTYPES = ("bf16", "fp8")
SWITCHES = {                                                 # one at a time against the defaults
    "default": {},
    "no_fuse_decode_rope": dict(fuse_decode_rope=False),
    "no_fuse_decode_norms": dict(fuse_decode_norms=False),
    "no_decode_packed_weights": dict(decode_packed_weights=False),
    "no_prefill_last_rows": dict(prefill_last_rows=False),
    "no_decode_t256": dict(decode_t256=()),
}
DECODE_BATCHES = (1, 8, 9, 64, 65, 128, 129, 256, 257)       # plan boundaries, the fused-RoPE threshold (8), the LoRA kernel switch (64)
# (name, seq_lens, with a cache, last_rows_only, last_out given); 16 x 376 = 6016 rows put the QKV GEMM on the 256 tile
PREFILLS = (
    ("last_5", [5], True, True, False),
    ("last_376x16_out", [376] * 16, True, True, True),
    ("last_376x16", [376] * 16, True, True, False),
    ("full_cache_ragged", [376, 3, 200] * 6, True, False, False),
    ("full_nocache_7_9", [7, 9], False, False, False),
    ("full_nocache_376x16", [376] * 16, False, False, False),
)


def _modules():
    from icl_speech_text_llm_amd.runtime import binding, config, engines, packing
    return binding, config, engines, packing


def configs():
    _, C, _, _ = _modules()
    base = replace(C.SalmonnCfg.llama2_7b().llama, n_layers=2)
    return {
        "7b_lora": base,
        "7b_nolora": replace(base, lora_rank=0),
        "7b_gqa8_bias": replace(base, n_kv_heads=8, qkv_bias=True),
        "tiny_h4": replace(C.SalmonnCfg.tiny().llama, n_heads=4, n_layers=2),    # head_dim 64: no fused RoPE epilogue
    }


def groups():
    """(config, weight mode, KV dtype, switch) of every group; the FP8 KV cache refuses a grouped-query decoder by design."""
    for cname, cfg in configs().items():
        for wm in WEIGHT_MODES:
            for kv in KV_DTYPES:
                if kv == "fp8" and cfg.group > 1:
                    continue
                for sw in SWITCHES:
                    yield cname, wm, kv, sw


def device_ok() -> bool:
    """The trace depends on the library's tile choice, which depends on the CU count: 256 on an MI355X and without a device."""
    B = _modules()[0]
    n = B.load_library().icl_device_cu_count()
    return n <= 0 or n == N_CU


# ---- the runtime under trace ------------------------------------------------------------------------------------------------
def _e(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device="meta")


def make_runtime(cfg, weight_mode: str, switches: dict):
    _, _, E, P = _modules()
    f32, u8 = torch.float32, torch.uint8
    hd, I, k_aug, nq = cfg.hidden, cfg.ffn, P.llama_k_aug(cfg), P.qkv_width(cfg)
    shapes = E.site_shapes(cfg, k_aug)
    layers = []
    for _ in range(cfg.n_layers):
        L = P.LlamaLayer(rms1=_e(hd, dtype=f32), bqkv=_e(nq, dtype=f32) if cfg.qkv_bias else None, wqkv=_e(nq, k_aug),
                         lora_a=_e(len(cfg.lora_targets) * cfg.lora_rank, hd) if cfg.lora_rank else None, wo=_e(hd, hd),
                         rms2=_e(hd, dtype=f32), wgu=_e(2 * I, hd), wdown=_e(hd, I))
        L.decode_packed = tuple(_e(-(-N // 16) * 16, K) for N, K in (shapes[s] for s in E.DECODE_SITES))
        if weight_mode == "fp8":
            L.fp8 = tuple((_e(-(-N // 16) * 16, K, dtype=u8), _e(N, dtype=f32)) for N, K in (shapes[s] for s in E.DECODE_SITES))
        layers.append(L)
    w = P.PackedLlama(cfg=cfg, embed=_e(cfg.vocab, hd), layers=layers, norm=_e(hd, dtype=f32), lm_head=_e(cfg.vocab, hd),
                      k_aug=k_aug, rope_cos=_e(cfg.max_pos, cfg.head_dim // 2, dtype=f32),
                      rope_sin=_e(cfg.max_pos, cfg.head_dim // 2, dtype=f32))
    rt = object.__new__(E.LlamaHIP)
    rt.w, rt.device, rt.n_cu, rt.weight_dtype = w, torch.device("meta"), N_CU, weight_mode
    for k, v in switches.items():
        setattr(rt, k, v)
    return rt


# ---- recorder ---------------------------------------------------------------------------------------------------------------
class Recorder:
    """One case: the launch log, the workspace requests, the storages numbered so far and the host-built index tensors."""

    def __init__(self):
        self.log = []
        self.requests = {}          # (name, dtype, zero, inner dims) -> largest numel
        self.storages = {}          # StorageImpl address -> (ordinal, the storage: kept alive, or addresses would be reused)
        self.host_index = {}        # id(tensor) -> (values, the tensor: kept alive for the same reason)

    def enc(self, x):
        if x is None or isinstance(x, (bool, int, str)):
            return repr(x)
        if isinstance(x, float):
            return repr(float(x))
        if isinstance(x, (tuple, list)):
            return "(" + ", ".join(self.enc(v) for v in x) + ")"
        if isinstance(x, torch.Generator):
            return "generator"
        if type(x).__name__ in ("BeamState", "DeviceTables"):      # by their fields; uid is a process-global counter
            return type(x).__name__ + "{" + ", ".join(f"{k}={self.enc(v)}" for k, v in sorted(vars(x).items()) if k != "uid") + "}"
        if isinstance(x, torch.Tensor):
            if id(x) in self.host_index:
                return "i32" + repr(self.host_index[id(x)][0]).replace(" ", "")
            if x.device.type != "meta":                            # a host table: by value
                return f"host:{str(x.dtype).replace('torch.', '')}{x.tolist()!r}".replace(" ", "")
            st = x.untyped_storage()
            ordinal = self.storages.setdefault(st._cdata, (len(self.storages), st))[0]
            return (f"T{ordinal}:{str(x.dtype).replace('torch.', '')}{list(x.shape)}/{list(x.stride())}+{x.storage_offset()}"
                    .replace(" ", ""))
        raise TypeError(f"launch argument of a type the trace cannot encode: {type(x).__name__}")

    def text(self) -> str:
        ws = sorted(f"ws {n} {str(d).replace('torch.', '')} zero={z} inner={','.join(map(str, inner))} numel={numel}"
                    for (n, d, z, inner), numel in self.requests.items())
        return "\n".join(self.log + ws) + "\n"


@contextlib.contextmanager
def recording(rec: Recorder):
    """Every launching wrapper of runtime.binding appends (name, bound arguments) to ``rec.log``; ``_i32`` (engines', under
    every runtime module that holds the name) remembers the values it was given, so index tensors built on the host are
    recorded by value."""
    B, _, E, _ = _modules()
    pkg = E.__name__.rsplit(".", 1)[0]
    importlib.import_module(pkg + ".salmonn")
    holders = [m for n, m in sorted(sys.modules.items()) if n.startswith(pkg + ".") and "_i32" in vars(m)]
    names = [n for n, f in vars(B).items() if inspect.isfunction(f) and f.__module__ == B.__name__ and not n.startswith("_")
             and n not in NOT_LAUNCHES]
    saved = {n: getattr(B, n) for n in names}
    real_i32 = E._i32

    def wrapper(name, real):
        sig = inspect.signature(real)

        def record(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            rec.log.append(f"{name}(" + ", ".join(f"{k}={rec.enc(v)}" for k, v in bound.arguments.items()) + ")")
            return bound.arguments["out"] if name in RETURNS_OUT else None
        return record

    def i32(x, device):
        values = [int(v) for v in x]
        t = real_i32(values, device)
        rec.host_index[id(t)] = (values, t)
        return t

    try:
        for n, f in saved.items():
            setattr(B, n, wrapper(n, f))
        for m in holders:
            m._i32 = i32
        yield rec
    finally:
        for n, f in saved.items():
            setattr(B, n, f)
        for m in holders:
            m._i32 = real_i32


def traced_workspace(rec: Recorder):
    E = _modules()[2]

    class TracedWorkspace(E.Workspace):
        def get(self, name, shape, dtype, zero=False):
            shape = tuple(int(s) for s in shape)
            numel = 1
            for s in shape:
                numel *= s
            key = (name, dtype, bool(zero), shape[1:])
            rec.requests[key] = max(rec.requests.get(key, 0), numel)
            return super().get(name, shape, dtype, zero=zero)

        def release(self, *names):
            rec.log.append("ws.release(" + ", ".join(names) + ")")
            super().release(*names)
    return TracedWorkspace("meta")


# ---- cases ------------------------------------------------------------------------------------------------------------------
def run_decode(rt, kv: str, Bn: int) -> str:
    E = _modules()[2]
    rec = Recorder()
    ws = traced_workspace(rec)
    with recording(rec):
        cache = E.KVCache(rt.w.cfg, Bn, CACHE_LEN, ws, dtype=kv)
        ids, pos, lens, sid = (_e(Bn, dtype=torch.int32) for _ in range(4))
        rt.decode_step(ws, cache, ids, pos, lens, sid)
    return rec.text()


def run_prefill(rt, kv: str, seq_lens, with_cache: bool, last_rows_only: bool, give_out: bool) -> str:
    E = _modules()[2]
    rec = Recorder()
    ws = traced_workspace(rec)
    hidden = rt.w.cfg.hidden
    with recording(rec):
        cache = E.KVCache(rt.w.cfg, len(seq_lens), CACHE_LEN, ws, dtype=kv) if with_cache else None
        h = _e(sum(seq_lens), hidden, dtype=torch.float32)
        last_out = _e(len(seq_lens), hidden, dtype=torch.float32) if give_out else None
        out = rt.prefill(ws, h, seq_lens, cache, last_rows_only=last_rows_only, last_out=last_out)
        rt.logits(ws, out)
    return rec.text()


def group_cases(cname: str, wm: str, kv: str, sw: str):
    """(case name, canonical text) of every case of one group, in a fixed order."""
    rt = make_runtime(configs()[cname], wm, SWITCHES[sw])
    for Bn in DECODE_BATCHES:
        yield f"decode_{Bn}", run_decode(rt, kv, Bn)
    for name, lens, with_cache, last, give_out in PREFILLS:
        yield f"prefill_{name}", run_prefill(rt, kv, lens, with_cache, last, give_out)


def digests(dump_dir=None):
    out = {}
    for g in groups():
        key = "/".join(g)
        text = "".join(f"== {name}\n{body}" for name, body in group_cases(*g))
        out[key] = hashlib.sha256(text.encode()).hexdigest()
        if dump_dir is not None:
            with open(os.path.join(dump_dir, key.replace("/", "__") + ".txt"), "w") as f:
                f.write(text)
    return out


# ---- the generation driver under trace --------------------------------------------------------------------------------------
GEN_LENS = (5, 9, 7, 4, 6)                                   # prompt lengths, in positions


class Plumbing(TorchDispatchMode):
    """Logs every in-place aten op and every ``clone`` whose first argument is a ``meta`` tensor (zero_, fill_, copy_, uniform_,
    index_put_, ...): what generate() does to device buffers between the launches."""

    def __init__(self, rec: Recorder):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = func._schema.name.split("::")[1]
        if (name.endswith("_") or name == "clone") and args and isinstance(args[0], torch.Tensor) and args[0].device.type == "meta":
            enc = [self.rec.enc(a) for a in args] + [f"{k}={self.rec.enc(v)}" for k, v in sorted(kwargs.items())]
            self.rec.log.append(f"torch.{name}(" + ", ".join(enc) + ")")
        return func(*args, **kwargs)


class Mark:
    """Stands in for a torch.cuda.Event of ``phase_marks``."""

    def __init__(self, rec: Recorder, name: str):
        self.rec, self.name = rec, name

    def record(self):
        self.rec.log.append(f"mark {self.name}")


@contextlib.contextmanager
def meta_cpu_reads_zeros():
    had, real = "cpu" in vars(torch.Tensor), torch.Tensor.cpu

    def cpu(self, *a, **kw):
        return torch.zeros(self.shape, dtype=self.dtype) if self.device.type == "meta" else real(self, *a, **kw)
    torch.Tensor.cpu = cpu
    try:
        yield
    finally:
        if had:
            torch.Tensor.cpu = real
        else:
            del torch.Tensor.cpu


@contextlib.contextmanager
def generate_recording(rec: Recorder):
    with recording(rec), meta_cpu_reads_zeros(), Plumbing(rec):
        yield rec


def prompts_of(lens=GEN_LENS):
    return [[list(range(3 + b, 3 + b + n))] for b, n in enumerate(lens)]


def _automaton():
    """0 -10-> 1 -11-> 2, 0 -12-> 2, 2 accepting (EOS id 2)."""
    from icl_speech_text_llm_amd.runtime.constraints import LabelAutomaton
    return LabelAutomaton([0, 2, 3, 4], [10, 12, 11, 2], [1, 2, 2, 2], {}, 260, 2)


def segments_of(lens):
    """Four segments per prompt, in position order."""
    return [[j * 4 // n for j in range(n)] for n in lens]


def _overlong_third(cfg):
    return (5, 9, cfg.max_pos + 119, 4, 6)


# name -> (attributes set on the runtime, prompt lengths, keyword arguments of generate()); a callable is built per run from
# (the decoder's cfg, the prompt lengths) — the lengths themselves from the cfg
GEN_CASES = {
    "greedy4": ({}, GEN_LENS, dict(max_new_tokens=4)),
    "greedy1": ({}, GEN_LENS, dict(max_new_tokens=1)),
    "chunk2": (dict(prefill_chunk=2), GEN_LENS, dict(max_new_tokens=4)),
    "chunk5": (dict(prefill_chunk=5), GEN_LENS, dict(max_new_tokens=4)),
    "eos_pair_pad": ({}, GEN_LENS, dict(max_new_tokens=4, eos_id=[2, 7], pad_id=5)),
    "suppress_eos": ({}, GEN_LENS, dict(max_new_tokens=4, suppress_eos=True)),
    "first_and_step_logits": ({}, GEN_LENS, dict(max_new_tokens=4, want_first_logits=True, want_step_logits=True)),
    "sample_seeded": ({}, GEN_LENS, dict(max_new_tokens=4, do_sample=True, top_k=5, top_p=0.9, temperature=0.7,
                                         generator=lambda cfg, lens: torch.Generator().manual_seed(1234))),
    "sample_global": ({}, GEN_LENS, dict(max_new_tokens=4, do_sample=True, top_k=5, top_p=0.9, temperature=0.7)),
    "sample_top_k0": ({}, GEN_LENS, dict(max_new_tokens=4, do_sample=True, top_k=0, top_p=0.9, temperature=0.7)),
    "repetition_penalty": ({}, GEN_LENS, dict(max_new_tokens=4, repetition_penalty=1.2)),
    "constrained": ({}, GEN_LENS, dict(max_new_tokens=4, constraint=lambda cfg, lens: (_automaton(), [0, -1, 1, 0, -1]))),
    "drop_overlong": ({}, (5, 9, 2167, 4, 6), dict(max_new_tokens=4, overlong="drop", want_first_logits=True)),
    "speech_segment": ({}, GEN_LENS, dict(max_new_tokens=4)),
    "beam3": ({}, GEN_LENS[:2], dict(max_new_tokens=3, num_beams=3)),
    "beam3_three_passes": (dict(beam_rows=6), GEN_LENS, dict(max_new_tokens=3, num_beams=3)),
    "beam3_repetition_penalty": ({}, GEN_LENS[:2], dict(max_new_tokens=3, num_beams=3, repetition_penalty=1.3)),
}
GEN_MATRIX = ([("tiny_h4", "bf16", name) for name in GEN_CASES]
              + [(cname, kv, name) for cname, kv in (("tiny_h4", "fp8"), ("7b_gqa8_bias", "bf16")) for name in ("greedy4", "beam3")])

# The probes of the deciding rows.  tiny_h4: head_dim 64, an untrimmed last layer; 7b_lora: the trimmed last layer with the
# suffix-query attention; 7b_gqa8_bias: grouped-query, untrimmed.  Each case once unchunked and once with prefill_chunk=2: rows 0
# and 3 of five then fall into the first two of three chunks, and the third chunk lists no row.
_PROBES = {
    "knockout": dict(knockout=lambda cfg, lens: (segments_of(lens), [[1], [], [], [0, 2], []], (1, 2), [1, 3])),
    "hidden": dict(want_hidden=True),
    "patch_all_steps": dict(patch=lambda cfg, lens: dict(site=1, vectors=torch.zeros(5, cfg.hidden), mode="add", alpha=0.5,
                                                         steps="all", rows=[0, 3])),
    "patch_last_site": dict(patch=lambda cfg, lens: dict(site=cfg.n_layers, vectors=torch.zeros(5, cfg.hidden), rows=[0, 3])),   # no capture
    "hidden_patch_shared": dict(want_hidden=True,          # the shared vector, all rows: capture and patch in one launch
                                patch=lambda cfg, lens: dict(site=cfg.n_layers, vectors=torch.zeros(1, cfg.hidden))),
    "heads": dict(want_heads=True),
    "head_patch_all_steps": dict(head_patch=lambda cfg, lens: dict(heads=[(1, 2), (0, 1), (1, 0)],       # two layers, out of order
                                                                   vectors=torch.zeros(5, 3, cfg.head_dim), mode="add", alpha=0.5,
                                                                   steps="all", rows=[0, 3])),
    "heads_patch_shared": dict(want_heads=True,            # shared vectors, all rows: capture and patch in one launch
                               head_patch=lambda cfg, lens: dict(heads=[(1, 2), (1, 0)], vectors=torch.zeros(1, 2, cfg.head_dim))),
    # interior rows (segment 1) and the last rows (segment 3) are listed, two heads of four or more, both layers — the last one
    # launches the last rows only — and the generated rows query as segment 1, so every decode step launches
    "cuts": dict(cuts=lambda cfg, lens: dict(segments=segments_of(lens), pairs=[(1, 0), (3, 0)], layers=(0, cfg.n_layers),
                                             heads=[0, 2], generated=1)),
}
PROBE_CASES = {}
for _name, _kw in _PROBES.items():
    PROBE_CASES[_name] = ({}, GEN_LENS, dict(max_new_tokens=4, **_kw))
    PROBE_CASES[_name + "_chunk2"] = (dict(prefill_chunk=2), GEN_LENS, dict(max_new_tokens=4, **_kw))
# overlong="drop" re-slices a probe to the kept rows: a knockout whose dropped row has a non-empty set, and a patch whose rows
# list the dropped row and one kept row
PROBE_CASES["drop_knockout"] = ({}, _overlong_third, dict(max_new_tokens=4, overlong="drop", knockout=lambda cfg, lens: (
    segments_of(lens), [[1], [], [2], [0, 2], []], (1, 2), [1, 3])))
PROBE_CASES["drop_hidden_patch"] = ({}, _overlong_third, dict(max_new_tokens=4, overlong="drop", want_hidden=True,
                                                              patch=lambda cfg, lens: dict(site=1, vectors=torch.zeros(5, cfg.hidden),
                                                                                           rows=[2, 3])))
# ... cuts with one pair list per prompt, the dropped one's too, and a head patch whose rows list the dropped row and one kept row
PROBE_CASES["drop_cuts"] = ({}, _overlong_third, dict(max_new_tokens=4, overlong="drop", cuts=lambda cfg, lens: dict(
    segments=segments_of(lens), pairs=[[(1, 0)], [(2, 1)], [(1, 0), (2, 0), (3, 0)], [(3, 1)], []], generated=[1, 3, 3, 3, 0])))
PROBE_CASES["drop_head_patch"] = ({}, _overlong_third, dict(max_new_tokens=4, overlong="drop", want_heads=True,
                                                            head_patch=lambda cfg, lens: dict(heads=[(1, 2), (0, 1)], rows=[2, 3],
                                                                                              vectors=torch.zeros(5, 2, cfg.head_dim))))
GEN_CASES.update(PROBE_CASES)
# prompt_attention(): name -> (attributes set on the runtime, its keyword arguments besides the segments)
PA_CASES = {
    "prompt_attention": ({}, {}),
    "prompt_attention_chunk2": (dict(prefill_chunk=2), {}),
    "prompt_attention_probs": ({}, dict(want_probs=True)),
    "prompt_attention_probs_chunk2": (dict(prefill_chunk=2), dict(want_probs=True)),
}
GEN_MATRIX += [(cname, "bf16", name) for cname in ("tiny_h4", "7b_lora", "7b_gqa8_bias") for name in (*PA_CASES, *PROBE_CASES)]
GEN_MATRIX += [("tiny_h4", "fp8", name) for name in ("patch_all_steps", "hidden")]      # patching works on both KV dtypes


def generate_runtime(cname: str, kv: str, rec: Recorder):
    """A SalmonnRuntime over ``make_runtime``'s decoder and a traced workspace, on ``meta``, without graphs; its phase marks log."""
    E = _modules()[2]
    S = importlib.import_module(E.__name__.rsplit(".", 1)[0] + ".salmonn")
    cfg = configs()[cname]
    rt = object.__new__(S.SalmonnRuntime)
    rt.lm_cfg, rt.llama, rt.ws, rt.device = cfg, make_runtime(cfg, "bf16", {}), traced_workspace(rec), torch.device("meta")
    rt.use_graphs, rt.kv_dtype = False, kv
    rt.phase_marks = {n: Mark(rec, n) for n in ("prefill_start", "prefill_end", "decode_end")}
    return rt


def _result_line(res) -> str:
    out = []
    for f in fields(res):
        v = getattr(res, f.name)
        out.append(f"{f.name}=" + (f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}@{v.device.type}" if isinstance(v, torch.Tensor)
                                   else repr(v)))
    return "result " + " ".join(out)


def run_prompt_attention(cname: str, kv: str, name: str) -> str:
    """The canonical text of one prompt_attention() call over GEN_LENS, four segments per prompt."""
    attrs, kw = PA_CASES[name]
    rec = Recorder()
    rt = generate_runtime(cname, kv, rec)
    for k, v in attrs.items():
        setattr(rt, k, v)
    with generate_recording(rec):
        res = rt.prompt_attention(prompts_of(), None, segments_of(GEN_LENS), **kw)
    rec.log.append(_result_line(res))
    return rec.text()


def run_generate(cname: str, kv: str, name: str) -> str:
    """The canonical text of one generate() call: launches, plumbing and marks in order, workspace requests, the result."""
    if name in PA_CASES:
        return run_prompt_attention(cname, kv, name)
    attrs, lens, kw = GEN_CASES[name]
    rec = Recorder()
    rt = generate_runtime(cname, kv, rec)
    lens = lens(rt.lm_cfg) if callable(lens) else lens
    kw = {k: v(rt.lm_cfg, lens) if callable(v) else v for k, v in kw.items()}
    for k, v in attrs.items():
        setattr(rt, k, v)
    prompts, speech = prompts_of(lens), None
    if name == "speech_segment":                                # row 0: two token ids, then speech rows 1..3
        prompts[0], speech = [[3, 4], ("speech", 1, 3)], _e(1, 8, rt.lm_cfg.hidden, dtype=torch.float32)
    with generate_recording(rec):
        res = rt.generate(prompts, speech, **kw)
    rec.log.append(_result_line(res))
    return rec.text()


def generate_digests(dump_dir=None):
    out = {}
    for case in GEN_MATRIX:
        key, text = "/".join(case), run_generate(*case)
        out[key] = hashlib.sha256(text.encode()).hexdigest()
        if dump_dir is not None:
            with open(os.path.join(dump_dir, "generate__" + key.replace("/", "__") + ".txt"), "w") as f:
                f.write(text)
    return out


def load_fixture(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate the fixture")
    ap.add_argument("--dump", metavar="DIR", help="write the full text of every case, one file per group")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is traced (default: this one)")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root))
    if not device_ok():
        print(f"the device does not have {N_CU} CUs: the fixture does not apply", file=sys.stderr)
        return 2
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    bad = []
    for what, path, got in (("groups", FIXTURE, digests(a.dump)), ("generate cases", GEN_FIXTURE, generate_digests(a.dump))):
        if a.write:
            with open(path, "w") as f:
                json.dump(got, f, indent=1, sort_keys=True)
                f.write("\n")
            print(f"wrote {len(got)} digests ({what})")
            continue
        want = load_fixture(path)
        differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        for k in differ:
            print("differs:", k)
        print(f"{len(got) - len([k for k in differ if k in got])} of {len(got)} {what} match")
        bad += differ
    return 1 if bad else 0

if __name__ == "__main__":
    sys.exit(main())
