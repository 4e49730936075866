"""Attention-head output capture and patching against what it rides on, one process, interleaved rounds.

Launch legs: icl_head_rows_bf16 on the last rows of an attention output of 256 prompts x 376 positions x 32 heads x 128 (bf16, 0.8
GB: every launch reads rows 3 MB apart), at 256 listed rows and at 1: capture only, replace of all 32 heads, capture + replace, add.
Bytes moved, from the shapes, in operands of n_rows x 4096 elements: a capture 2 x 2 bytes (att in, capture out), a replace 4 + 2
(f32 vectors in, att out), capture + replace 4 + 3 x 2, an add 4 + 2 x 2.  The expectation from the code alone is that a launch is
bound by its latency, not by those bytes; the leg next to it is icl_gather_rows_bf16 over the same rows, which moves what a capture
moves.
Runtime leg: ``generate(max_new_tokens=8)`` on the 2-layer decoder of tools/bench_resid_patch.py (Llama-2-7B's layer shape: hidden
4096, 32 heads, ffn 11008, vocab 32000; synthetic weights), 256 prompts of 373-376 positions: the plain call (nothing new is
launched), with ``want_heads``, and with an add patch of four heads in both layers with ``steps="all"`` — wall time per call, host
syncs included.

    python tools/bench_head_patch.py [--rounds 5] [--reps 30] [--out profiles/r16_head_patch.json] [--no-runtime]
Run each invocation under a time limit of its own (``timeout -k 10 300 python tools/bench_head_patch.py``).
Prints one line per measurement and a JSON summary (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import time
from dataclasses import replace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS, HEAD_DIM, SEQS, POSITIONS = 32, 128, 256, 376
HIDDEN = HEADS * HEAD_DIM
NEW_TOKENS = 8


def _time(fn, reps, out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        fn(i)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]


def launch_leg(n, rounds, reps):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    att = torch.randn(SEQS * POSITIONS, HIDDEN, device=dev).to(torch.bfloat16)
    rows = (torch.arange(n, dtype=torch.int32, device=dev) + 1) * POSITIONS - 1          # the prompts' last rows
    cap = torch.empty(n, HIDDEN, dtype=torch.bfloat16, device=dev)
    heads = torch.arange(HEADS, dtype=torch.int32, device=dev)
    vec = torch.randn(n, HEADS, HEAD_DIM, device=dev) * 0.01
    kw = dict(n_heads=HEADS, head_dim=HEAD_DIM)
    elems = n * HIDDEN
    modes = {        # name -> (launch, bytes it moves)
        "gather_rows": (lambda i: B.gather_rows(att, rows, cap), 4 * elems),
        "capture": (lambda i: B.head_rows(att, rows, capture=cap, **kw), 4 * elems),
        "replace": (lambda i: B.head_rows(att, rows, heads=heads, vec=vec, **kw), 6 * elems),
        "capture_replace": (lambda i: B.head_rows(att, rows, capture=cap, heads=heads, vec=vec, **kw), 10 * elems),
        "add": (lambda i: B.head_rows(att, rows, heads=heads, vec=vec, mode="add", alpha=0.5, **kw), 8 * elems),
    }
    times = {m: [] for m in modes}
    for fn, _ in modes.values():
        fn(0)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for m, (fn, _) in modes.items():
            _time(fn, reps, times[m])
    recs = []
    for m, ts in times.items():
        us = statistics.median(ts)
        moved = modes[m][1]
        rec = {"n_rows": n, "n_heads": HEADS, "head_dim": HEAD_DIM, "launch": m, "us_median": round(us, 2), "us_min": round(min(ts), 2),
               "bytes_moved": moved, "eff_gb_s": round(moved / us / 1e3, 1)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def runtime_leg(rounds):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    tiny = SalmonnCfg.tiny(use_beats=False)
    cfg = replace(tiny, llama=replace(tiny.llama, hidden=HIDDEN, n_layers=2, n_heads=HEADS, ffn=11008, vocab=32000, max_pos=4096, pad_id=0))
    rt = SalmonnRuntime(cfg, synth.salmonn_state(cfg, seed=0, parts=("llama",)), device="cuda", parts=("llama",), consume=True)
    g = torch.Generator().manual_seed(5)
    lens = [373 + b % 4 for b in range(SEQS)]
    prompts = [[torch.randint(3, 31999, (n,), generator=g).tolist()] for n in lens]
    pairs = [(0, 3), (0, 17), (1, 5), (1, 30)]
    vec = torch.randn(SEQS, len(pairs), HEAD_DIM, generator=g).to("cuda") * 0.05
    kw = dict(max_new_tokens=NEW_TOKENS, suppress_eos=True)
    modes = {
        "generate": lambda: rt.generate(prompts, None, **kw),
        "generate_want_heads": lambda: rt.generate(prompts, None, want_heads=True, **kw),
        "generate_head_add_all": lambda: rt.generate(prompts, None, head_patch=dict(heads=pairs, vectors=vec, mode="add", alpha=0.5, steps="all"), **kw),
    }
    times = {m: [] for m in modes}
    for fn in modes.values():            # twice: the second call captures the decode graph
        fn()
        fn()
    for _ in range(rounds):
        for m, fn in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) * 1e3)
    rec = {"n_layers": cfg.llama.n_layers, "hidden": cfg.llama.hidden, "n_heads": cfg.llama.n_heads, "n_seqs": len(lens),
           "positions": [min(lens), max(lens)], "new_tokens": NEW_TOKENS, "prefill_chunk": rt.prefill_chunk, "patched_pairs": pairs,
           **{m + "_ms_median": round(statistics.median(ts), 3) for m, ts in times.items()},
           **{m + "_ms_min": round(min(ts), 3) for m, ts in times.items()},
           "generate_ms_spread": round(max(times["generate"]) - min(times["generate"]), 3)}
    for m in list(modes)[1:]:
        rec[m + "_minus_generate_ms"] = round(rec[m + "_ms_median"] - rec["generate_ms_median"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_head_patch.json"))
    ap.add_argument("--no-runtime", action="store_true")
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "legs": []}
    for n in (SEQS, 1):
        res["legs"] += launch_leg(n, args.rounds, args.reps)
        torch.cuda.empty_cache()
    if not args.no_runtime:
        res["runtime"] = runtime_leg(args.rounds)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
