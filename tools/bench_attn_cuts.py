"""Attention cuts between prompt segments against the launch they rewrite, one process, interleaved rounds.

Kernel legs: icl_attn_cut_rows_bf16 at head_dim 128, 32 heads and 32 / 8 heads, 256 sequences of 385 keys (cache length 448), with 8
and with 64 listed rows per sequence, spread evenly over the prompt — in the form's tiles (R rows of one sequence share one pass over
its K / V) and, where R > 1, the same list with every row alone in a tile — next to icl_attn_fwd_bf16 over the same prompts from the
same cache, the launch whose rows are rewritten.  A tile streams its sequence's K / V up to its longest row once, so the bytes
requested are the sum over tiles of Hkv * 2 * (longest row_len) * head_dim * 2; tiles of one sequence re-read the same 100-200 KB per
head, and how much of that L2 absorbs shows in the effective rate.  The caches rotate through more than the 256 MiB Infinity Cache.
Runtime leg: ``generate(max_new_tokens=8)`` with and without cuts on a 2-layer decoder of Llama-2-7B's layer shape (hidden 4096, 32
heads, ffn 11008, vocab 32000; synthetic weights), 256 prompts of 373-376 positions in 8 segments, pairs (2, 1), (4, 3), (6, 5) —
three eighths of every prompt's rows listed in layer 0, none in the last layer, the generated rows untouched: wall time per call.

    python tools/bench_attn_cuts.py [--rounds 5] [--reps 10] [--out profiles/r17_attn_cuts.json] [--no-runtime]
Run each invocation under a time limit of its own (``timeout -k 10 300 python tools/bench_attn_cuts.py``).
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

D, T, LIVE, N_SEG, N_SEQS = 128, 448, 385, 8, 256
SHAPES = ((32, 32), (32, 8))
LISTED = (8, 64)
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


def _tables(n, k, R, alone, dev):
    """k listed positions per sequence, evenly spread, segment 3 of 8 cut for each; tiles of R consecutive entries (``alone``: one
    live slot per tile).  Returns (tile_seq, row_q, row_len, blocked, sum over tiles of the longest row_len)."""
    pos = [(i + 1) * LIVE // k - 1 for i in range(k)]
    tile_seq, row_q, row_len, blocked, keys = [], [], [], [], 0
    step = 1 if alone else R
    for b in range(n):
        for i in range(0, k, step):
            part = pos[i:i + step]
            pad = R - len(part)
            tile_seq.append(b)
            row_q += [b * LIVE + p for p in part] + [-1] * pad
            row_len += [p + 1 for p in part] + [0] * pad
            blocked += [1 << 3] * len(part) + [0] * pad
            keys += part[-1] + 1
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    return i32(tile_seq), i32(row_q), i32(row_len), i32(blocked), keys


def kernel_leg(H, Hkv, rounds, reps):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    n, R = N_SEQS, B.attn_cut_tile_rows(H, D, Hkv)
    copies = max(2, -(-2 * L3_BYTES // (n * Hkv * LIVE * D * 2 * 2)))
    kc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    vc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    q = (torch.randn(n * LIVE, H * D, device=dev) * 0.5).to(torch.bfloat16)
    o = torch.empty(n * LIVE, H * D, dtype=torch.bfloat16, device=dev)
    cu = torch.arange(n + 1, dtype=torch.int32, device=dev) * LIVE
    seg = (torch.arange(T, device=dev) * N_SEG // LIVE).clamp_max(255).to(torch.uint8)[None].repeat(n, 1).contiguous()
    scale = D ** -0.5
    if H == Hkv:          # as the runtime launches it: multi-head reads k / v from the cache, grouped-query from packed rows
        fwd = lambda i: B.attn_fwd(q, kc[i % copies], vc[i % copies], o, cu, LIVE, H, D, scale, causal=True, kv_cache_max_len=T)
    else:
        kp = [(torch.randn(n * LIVE, Hkv * D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(2 * copies)]
        fwd = lambda i: B.attn_fwd(q, kp[2 * (i % copies)], kp[2 * (i % copies) + 1], o, cu, LIVE, H, D, scale, causal=True, n_kv_heads=Hkv)
    modes = {"attn_fwd": (fwd, None)}
    for k in LISTED:
        for alone in ((False, True) if R > 1 else (False,)):
            ts, rq, rl, bl, keys = _tables(n, k, R, alone, dev)
            fn = (lambda ts, rq, rl, bl: lambda i: B.attn_cut_rows(q, kc[i % copies], vc[i % copies], o, seg, ts, rq, rl, bl, H, D, T, scale,
                                                                  tile_rows=R, n_kv_heads=Hkv))(ts, rq, rl, bl)
            modes[f"cut_rows_{k}_per_seq" + ("_alone" if alone else "")] = (fn, (k, int(ts.numel()), keys))
    times = {m: [] for m in modes}
    for fn, _ in modes.values():
        for i in range(copies):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for m, (fn, _) in modes.items():
            _time(fn, reps, times[m])
    recs = []
    for m, ts in times.items():
        us, info = statistics.median(ts), modes[m][1]
        rec = {"n_heads": H, "n_kv_heads": Hkv, "n_seqs": n, "live_keys": LIVE, "kernel": m, "us_median": round(us, 2), "us_min": round(min(ts), 2),
               "cache_copies_rotated": copies}
        if info is not None:
            k, n_tiles, keys = info
            req = keys * Hkv * 2 * D * 2
            rec.update(tile_rows=R, listed_rows=n * k, n_tiles=n_tiles, workgroups=n_tiles * Hkv, bytes_requested=req,
                       requested_tb_s=round(req / us / 1e6, 3), us_per_listed_row=round(us / (n * k), 4))
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
    lens = [373 + b % 4 for b in range(N_SEQS)]
    prompts = [[torch.randint(3, 31999, (n,), generator=g).tolist()] for n in lens]
    cuts = dict(segments=[[j * N_SEG // n for j in range(n)] for n in lens], pairs=[(2, 1), (4, 3), (6, 5)], generated=255)
    kw = dict(max_new_tokens=NEW_TOKENS, suppress_eos=True)
    modes = {"generate": lambda: rt.generate(prompts, None, **kw), "generate_cuts": lambda: rt.generate(prompts, None, cuts=cuts, **kw)}
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
    listed = sum(sum(1 for s in sg if s in (2, 4, 6)) for sg in cuts["segments"])
    rec = {"n_layers": cfg.llama.n_layers, "hidden": cfg.llama.hidden, "n_heads": cfg.llama.n_heads, "n_seqs": len(lens),
           "positions": [min(lens), max(lens)], "n_seg": N_SEG, "new_tokens": NEW_TOKENS, "listed_rows_layer_0": listed,
           **{m + "_ms_median": round(statistics.median(ts), 3) for m, ts in times.items()},
           **{m + "_ms_min": round(min(ts), 3) for m, ts in times.items()}}
    rec["cuts_minus_generate_ms"] = round(rec["generate_cuts_ms_median"] - rec["generate_ms_median"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_attn_cuts.json"))
    ap.add_argument("--no-runtime", action="store_true")
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "head_dim": D, "cache_len": T, "legs": []}
    for H, Hkv in SHAPES:
        res["legs"] += kernel_leg(H, Hkv, args.rounds, args.reps)
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
