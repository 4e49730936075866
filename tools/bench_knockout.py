"""Attention knockout against what it rides on, one process, interleaved rounds.

Kernel legs: icl_attn_decode_masked_bf16 (every row listed; 8 segments, one blocked in every head; and with every mask 0) against
the decode attention on the same cache — icl_attn_decode_bf16 at 32 heads, icl_attn_decode_gqa_bf16 at 32 / 8 heads — head_dim 128,
cache length 448 with 385 live keys, at 256 sequences and at 1.  The masked launch reads the bytes of a decode-attention launch plus
one segment byte per key.  Every launch streams its cache from HBM (the caches rotate through more than the 256 MiB Infinity Cache).
Runtime leg: ``generate(max_new_tokens=8)`` with and without a knockout of one segment in all layers and heads, on a 2-layer decoder
of Llama-2-7B's layer shape (hidden 4096, 32 heads, ffn 11008, vocab 32000; synthetic weights), 256 prompts of 373-376 positions in
8 segments: wall time per call, host syncs included (the knockout adds one launch per layer to the prefill chunks and to every
decode step, and takes the two-launch RoPE + attention form of the step).

    python tools/bench_knockout.py [--rounds 5] [--reps 30] [--out profiles/r13_knockout.json] [--no-runtime]
Run each invocation under a time limit of its own (``timeout -k 10 300 python tools/bench_knockout.py``).
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
NEW_TOKENS = 8


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
    nbytes = n * Hkv * LIVE * D * 2 * 2                      # K + V once
    copies = max(2, min(-(-2 * L3_BYTES // nbytes), (2 << 30) // (n * Hkv * T * D * 2 * 2)))
    kc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    vc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    q = (torch.randn(n, H * D, device=dev) * 0.5).to(torch.bfloat16)
    o = torch.empty(n, H * D, dtype=torch.bfloat16, device=dev)
    lens = torch.full((n,), LIVE, dtype=torch.int32, device=dev)
    seg = (torch.arange(T, device=dev) * N_SEG // LIVE).clamp_max(255).to(torch.uint8)[None].repeat(n, 1).contiguous()
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    one = torch.full((n, H), 1 << 3, dtype=torch.int32, device=dev)          # segment 3 of 8 blocked in every head
    none = torch.zeros(n, H, dtype=torch.int32, device=dev)
    scale = D ** -0.5
    if H == Hkv:
        decode = lambda i: B.attn_decode(q, kc[i % copies], vc[i % copies], o, lens, H, D, T, scale)
    else:
        decode = lambda i: B.attn_decode_gqa(q, kc[i % copies], vc[i % copies], o, lens, H, Hkv, D, T, scale)
    masked = lambda bl: (lambda i: B.attn_decode_masked(q, kc[i % copies], vc[i % copies], o, lens, seg, bl, rows, rows, H, D, T, scale,
                                                        n_kv_heads=Hkv))
    modes = {"decode_attention": decode, "masked_one_segment": masked(one), "masked_nothing_blocked": masked(none)}
    times = {m: [] for m in modes}
    for fn in modes.values():
        for i in range(copies):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for m, fn in modes.items():
            _time(fn, reps, times[m])
    recs = []
    for m, ts in times.items():
        us = statistics.median(ts)
        read = nbytes + (0 if m == "decode_attention" else n * Hkv * LIVE)
        rec = {"n_heads": H, "n_kv_heads": Hkv, "n_seqs": n, "live_keys": LIVE, "kernel": m, "us_median": round(us, 2),
               "us_min": round(min(ts), 2), "bytes_read": read, "eff_tb_s": round(read / us / 1e6, 3),
               "workgroups": n * Hkv, "cache_copies_rotated": copies}
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
    lens = [373 + b % 4 for b in range(256)]
    prompts = [[torch.randint(3, 31999, (n,), generator=g).tolist()] for n in lens]
    knockout = ([[j * N_SEG // n for j in range(n)] for n in lens], [[3]] * len(lens))
    kw = dict(max_new_tokens=NEW_TOKENS, suppress_eos=True)
    modes = {
        "generate": lambda: rt.generate(prompts, None, **kw),
        "generate_knockout": lambda: rt.generate(prompts, None, knockout=knockout, **kw),
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
           "positions": [min(lens), max(lens)], "n_seg": N_SEG, "new_tokens": NEW_TOKENS,
           **{m + "_ms_median": round(statistics.median(ts), 3) for m, ts in times.items()},
           **{m + "_ms_min": round(min(ts), 3) for m, ts in times.items()}}
    rec["knockout_minus_generate_ms"] = round(rec["generate_knockout_ms_median"] - rec["generate_ms_median"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_knockout.json"))
    ap.add_argument("--no-runtime", action="store_true")
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "head_dim": D, "cache_len": T, "legs": []}
    for H, Hkv in SHAPES:
        for n in (256, 1):
            res["legs"] += kernel_leg(H, Hkv, n, args.rounds, args.reps)
            torch.cuda.empty_cache()
    t = {(r["n_kv_heads"], r["n_seqs"], r["kernel"]): r["us_median"] for r in res["legs"]}
    res["summary"] = {f"{H}/{Hkv} heads, {n} seqs": {"decode_attention_us": t[(Hkv, n, "decode_attention")],
                                                     "masked_one_segment_us": t[(Hkv, n, "masked_one_segment")],
                                                     "masked_nothing_blocked_us": t[(Hkv, n, "masked_nothing_blocked")],
                                                     "masked_over_decode": round(t[(Hkv, n, "masked_one_segment")] / t[(Hkv, n, "decode_attention")], 3)}
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
