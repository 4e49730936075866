"""The segment-to-segment attention flow against the launch it sits beside, one process, interleaved rounds.

Kernel legs: icl_attn_segflow_bf16 (8 segments) against icl_attn_fwd_bf16 (causal, K / V read from the cache) over the same
prompts — head_dim 128, prompts of 385 positions, cache length 448, at 32 heads and at 32 / 8 heads, 256 sequences and 1.  Both
launches form the same causal QK^T; the flash launch then multiplies by V (head_dim wide), the flow launch by the one-hot segment
matrix (32 wide, twice: hi and lo) and never reads V.  Every launch streams its cache from HBM (the caches rotate through more than
the 256 MiB Infinity Cache).
Runtime leg: ``prompt_attention`` with and without ``want_flow`` on a 2-layer decoder of Llama-2-7B's layer shape (hidden 4096, 32
heads, ffn 11008, vocab 32000; synthetic weights), 256 prompts of 385 positions in 8 segments: wall time per call, host syncs
included.  With ``want_flow`` the call adds one flow launch per layer, the D2H copy of the flow, and runs its last layer at full
height instead of on the 256 last rows.

    python tools/bench_segflow.py [--rounds 5] [--reps 20] [--out profiles/r18_segflow.json] [--no-runtime]
Run each invocation under a time limit of its own (``timeout -k 10 300 python tools/bench_segflow.py``).
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

D, T, LIVE, N_SEG = 128, 448, 385, 8
SHAPES = ((32, 32), (32, 8))
L3_BYTES = 256 << 20


def _time(fn, reps, out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        fn(i)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]


def kernel_leg(H, Hkv, n, rounds, reps):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    kbytes = n * Hkv * LIVE * D * 2                          # the live K rows of one cache copy
    copies = max(2, min(-(-2 * L3_BYTES // (2 * kbytes)), (4 << 30) // (n * Hkv * T * D * 2 * 2)))
    kc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    vc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    q = (torch.randn(n * LIVE, H * D, device=dev) * 0.5).to(torch.bfloat16)
    o = torch.empty(n * LIVE, H * D, dtype=torch.bfloat16, device=dev)
    cu = torch.arange(n + 1, dtype=torch.int32, device=dev) * LIVE
    seg = (torch.arange(T, device=dev) * N_SEG // LIVE).clamp_max(255).to(torch.uint8)[None].repeat(n, 1).contiguous()
    flow = torch.empty(n, H, N_SEG, N_SEG, device=dev)
    scale = D ** -0.5
    modes = {
        "attn_fwd": lambda i: B.attn_fwd(q, kc[i % copies], vc[i % copies], o, cu, LIVE, H, D, scale, causal=True, kv_cache_max_len=T,
                                         n_kv_heads=0 if H == Hkv else Hkv),
        "segflow": lambda i: B.attn_segflow(q, cu, kc[i % copies], seg, flow, H, D, T, LIVE, scale, n_kv_heads=0 if H == Hkv else Hkv),
    }
    times = {m: [] for m in modes}
    for fn in modes.values():
        for i in range(copies):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for m, fn in modes.items():
            _time(fn, reps, times[m])
    pairs = LIVE * (LIVE + 1) // 2
    recs = []
    for m, ts in times.items():
        us = statistics.median(ts)
        rec = {"n_heads": H, "n_kv_heads": Hkv, "n_seqs": n, "positions": LIVE, "kernel": m, "us_median": round(us, 2),
               "us_min": round(min(ts), 2), "us_per_row_per_32_heads": round(us / (n * LIVE) * 32 / H, 4),
               "qk_tflops_causal": round(2 * D * pairs * n * H / us / 1e6, 1), "workgroups": n * H * (1 if m == "segflow" else -(-LIVE // 128)),
               "cache_copies_rotated": copies}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def runtime_leg(rounds):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    tiny = SalmonnCfg.tiny(use_beats=False)
    cfg = replace(tiny, llama=replace(tiny.llama, hidden=4096, n_layers=2, n_heads=32, ffn=11008, vocab=32000, max_pos=4096, pad_id=0))
    rt = SalmonnRuntime(cfg, synth.salmonn_state(cfg, seed=0, parts=("llama",)), device="cuda", parts=("llama",), consume=True)
    g = torch.Generator().manual_seed(5)
    lens = [LIVE] * 256
    prompts = [[torch.randint(3, 31999, (n,), generator=g).tolist()] for n in lens]
    segments = [[j * N_SEG // n for j in range(n)] for n in lens]
    modes = {
        "prompt_attention": lambda: rt.prompt_attention(prompts, None, segments),
        "prompt_attention_flow": lambda: rt.prompt_attention(prompts, None, segments, want_flow=True),
    }
    times = {m: [] for m in modes}
    for fn in modes.values():
        fn()
    for _ in range(rounds):
        for m, fn in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) * 1e3)
    rec = {"n_layers": cfg.llama.n_layers, "hidden": cfg.llama.hidden, "n_heads": cfg.llama.n_heads, "n_seqs": len(lens),
           "positions": LIVE, "n_seg": N_SEG,
           **{m + "_ms_median": round(statistics.median(ts), 3) for m, ts in times.items()},
           **{m + "_ms_min": round(min(ts), 3) for m, ts in times.items()}}
    # per call: two flow launches, the full-height last layer in place of the trimmed one, the D2H copy of the flow
    rec["flow_minus_plain_ms"] = round(rec["prompt_attention_flow_ms_median"] - rec["prompt_attention_ms_median"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_segflow.json"))
    ap.add_argument("--no-runtime", action="store_true")
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "head_dim": D, "cache_len": T, "positions": LIVE, "n_seg": N_SEG, "legs": []}
    for H, Hkv in SHAPES:
        for n in (256, 1):
            res["legs"] += kernel_leg(H, Hkv, n, args.rounds, args.reps)
            torch.cuda.empty_cache()
    t = {(r["n_kv_heads"], r["n_seqs"], r["kernel"]): r["us_median"] for r in res["legs"]}
    res["summary"] = {f"{H}/{Hkv} heads, {n} seqs": {"attn_fwd_us": t[(Hkv, n, "attn_fwd")], "segflow_us": t[(Hkv, n, "segflow")],
                                                     "segflow_over_attn_fwd": round(t[(Hkv, n, "segflow")] / t[(Hkv, n, "attn_fwd")], 3)}
                      for H, Hkv in SHAPES for n in (256, 1)}
    if not args.no_runtime:
        res["runtime"] = runtime_leg(args.rounds)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
