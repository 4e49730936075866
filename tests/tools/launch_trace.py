"""Launch trace of the Llama decoder runtime (runtime/engines.py: LlamaHIP.prefill / decode_step / logits), on the CPU.

What the decoder runtime DOES is the sequence of library launches it makes: the kernels are in libicl_hip, the Python only
chooses which to call, on which operands, in which order.  This tool runs the public methods of ``LlamaHIP`` over a matrix of
model shapes, weight / KV modes, switches and batch sizes with every launching wrapper of ``runtime.binding`` replaced by a
recorder, and reduces what it saw to one sha256 per (config, weight mode, KV dtype, switch) group.  Two versions of
engines.py with the same digests make the same calls with the same operands in the same order — bit-identical results and
the same device time by construction.  tests/test_launch_trace.py compares against tests/golden/llama_launch_trace.json.

Nothing is computed: the weights are ``torch.empty`` tensors on the ``meta`` device (real 7B dims cost no memory).  The only
library entry point reached is icl_gemm_select_tile (``binding.rope_fusable``), which needs the built library but no GPU.

    python tests/tools/launch_trace.py                 compare with the fixture, list the groups that differ
    python tests/tools/launch_trace.py --write         regenerate the fixture
    python tests/tools/launch_trace.py --dump DIR      also write the full text of every case, one file per group
    python tests/tools/launch_trace.py --root TREE     trace TREE's package instead of this tree's (another checkout of the
                                                       repository; ICL_LIB_PATH names the built library if TREE has none)

A digest that differs is diffed with two ``--dump`` directories, one per tree.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import inspect
import json
import os
import sys
from dataclasses import replace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(ROOT, "tests", "golden", "llama_launch_trace.json")

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
        if isinstance(x, torch.Tensor):
            if id(x) in self.host_index:
                return "i32" + repr(self.host_index[id(x)][0]).replace(" ", "")
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
    """Every launching wrapper of runtime.binding appends (name, bound arguments) to ``rec.log``; ``engines._i32`` remembers the
    values it was given, so index tensors built on the host are recorded by value."""
    B, _, E, _ = _modules()
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
        E._i32 = i32
        yield rec
    finally:
        for n, f in saved.items():
            setattr(B, n, f)
        E._i32 = real_i32


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


def load_fixture():
    with open(FIXTURE) as f:
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
    got = digests(a.dump)
    if a.write:
        with open(FIXTURE, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(got)} digests")
        return 0
    want = load_fixture()
    bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    for k in bad:
        print("differs:", k)
    print(f"{len(got) - len([k for k in bad if k in got])} of {len(got)} groups match")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
