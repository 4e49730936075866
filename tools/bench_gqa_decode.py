"""GQA decode attention vs the multi-head kernel on the per-group expanded cache, one process, interleaved rounds.

Both kernels compute the same query heads: icl_attn_decode_gqa_bf16 reads a cache of Hkv heads once per workgroup, for the
G = H / Hkv query heads that share each row; icl_attn_decode_bf16 reads the cache expanded to H heads.  Shapes: 32 / 8 heads
(Llama-3-8B, Mistral-7B) and 28 / 4 (Qwen2-7B), head_dim 128, cache length 448 with 385 live keys, at 256 sequences and at 1.
Per kernel: median and minimum us per launch, the cache bytes it reads and the effective TB/s of those bytes.  Every launch
streams its cache from HBM (the caches rotate through more than the 256 MiB Infinity Cache).

    python tools/bench_gqa_decode.py [--rounds 5] [--reps 30] [--out profiles/r07_gqa_decode.json]
Run each invocation under a time limit of its own (``timeout -k 10 300 python tools/bench_gqa_decode.py``).
Prints one line per measurement and a JSON summary (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, T, LIVE = 128, 448, 385
SHAPES = ((32, 8), (28, 4))
L3_BYTES = 256 << 20


def _time(fn, reps, out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        fn(i)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]


def leg(H, Hkv, n, rounds, reps):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    G = H // Hkv
    gqa_bytes = n * Hkv * LIVE * D * 2 * 2                   # K and V rows the GQA kernel reads per launch
    mha_bytes = gqa_bytes * G
    # enough rotating copies that neither kernel finds its cache in the Infinity Cache (at most 2 GiB per kernel)
    copies = max(2, min(-(-2 * L3_BYTES // gqa_bytes), (2 << 30) // (n * H * T * D * 2 * 2)))
    kc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    vc = [(torch.randn(n, Hkv, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    kx = [k.repeat_interleave(G, dim=1).contiguous() for k in kc]
    vx = [v.repeat_interleave(G, dim=1).contiguous() for v in vc]
    q = (torch.randn(n, H * D, device=dev) * 0.5).to(torch.bfloat16)
    o = torch.empty(n, H * D, dtype=torch.bfloat16, device=dev)
    o2 = torch.empty_like(o)
    lens = torch.full((n,), LIVE, dtype=torch.int32, device=dev)
    modes = {
        "gqa": lambda i: B.attn_decode_gqa(q, kc[i % copies], vc[i % copies], o, lens, H, Hkv, D, T, D ** -0.5),
        "mha_expanded": lambda i: B.attn_decode(q, kx[i % copies], vx[i % copies], o2, lens, H, D, T, D ** -0.5),
    }
    times = {m: [] for m in modes}
    for fn in modes.values():
        for i in range(copies):
            fn(i)
    torch.cuda.synchronize()
    equal = float((o.view(torch.int16) == o2.view(torch.int16)).float().mean())      # both ran copy (copies - 1) last
    for _ in range(rounds):
        for m, fn in modes.items():
            _time(fn, reps, times[m])
    recs = []
    for m, ts in times.items():
        us = statistics.median(ts)
        nbytes = gqa_bytes if m == "gqa" else mha_bytes
        rec = {"n_heads": H, "n_kv_heads": Hkv, "group": G, "n_seqs": n, "live_keys": LIVE, "kernel": m, "us_median": round(us, 2),
               "us_min": round(min(ts), 2), "cache_bytes_read": nbytes, "eff_tb_s": round(nbytes / us / 1e6, 3),
               "workgroups": n * (Hkv if m == "gqa" else H), "cache_copies_rotated": copies, "bit_equal_share": round(equal, 4)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "head_dim": D, "cache_len": T, "legs": []}
    for H, Hkv in SHAPES:
        for n in (256, 1):
            res["legs"] += leg(H, Hkv, n, args.rounds, args.reps)
            torch.cuda.empty_cache()
    t = {(r["n_heads"], r["n_seqs"], r["kernel"]): r["us_median"] for r in res["legs"]}
    res["summary"] = {f"{H}/{Hkv} heads, {n} seqs": {"gqa_us": t[(H, n, "gqa")], "mha_expanded_us": t[(H, n, "mha_expanded")],
                                                     "gqa_over_mha": round(t[(H, n, "gqa")] / t[(H, n, "mha_expanded")], 3)}
                      for H, Hkv in SHAPES for n in (256, 1)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
