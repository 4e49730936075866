"""icl_qknorm_rope_kv_bf16 vs icl_rope_kv_gqa_bf16 on the same buffers, one process, interleaved rounds.

Both kernels read and rewrite the q | k column blocks of a packed QKV buffer in place and append k / v to the cache; the first
adds the per-head RMSNorm of a QK-norm decoder (Qwen3) in front of the rotation: the same bytes, one shuffle reduction per head
row more.  Shape: 32 query / 8 K/V heads, head_dim 128 (Qwen3-8B), cache length 448, at M = 1 row, 256 rows (a decode step: one
new position per sequence) and 256 x 385 rows (the prefill of 256 prompts of 385 tokens).  Buffers rotate through more than the
256 MiB Infinity Cache where a launch moves enough bytes for that to matter (at most 64 copies: the M = 1 and M = 256 launches
are latency-bound and their few KiB / MiB stay cached — said in the record).  Both kernels run in place on the same rotating
buffers, so the data a launch sees has been rotated (and, for the norm kernel, normalised) by the launches before it; neither
kernel's time depends on the values.

    python tools/bench_qknorm.py [--rounds 5] [--reps 20] [--out profiles/r10_qknorm.json]
Run each invocation under a time limit of its own (``timeout -k 10 300 python tools/bench_qknorm.py``).
Prints one line per measurement and a JSON summary (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, HKV, D, T, LIVE, SEQS = 32, 8, 128, 448, 385, 256
L3_BYTES = 256 << 20
MAX_COPIES = 64


def _time(fn, reps, out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        fn(i)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]


def leg(M, rounds, reps):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    width = (H + 2 * HKV) * D
    k_off, v_off = H * D, (H + HKV) * D
    moved = M * (2 * (H + HKV) * D * 2 + HKV * D * 2 + 2 * HKV * D * 2)      # q, k read + written; v read; k, v appended
    copies = max(2, min(MAX_COPIES, -(-2 * L3_BYTES // moved), (3 << 30) // (M * width * 2)))
    bufs = [(torch.randn(M, width, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
    if M == SEQS * LIVE:
        pos = torch.arange(M, device=dev, dtype=torch.int32) % LIVE
        sid = (torch.arange(M, device=dev, dtype=torch.int32) // LIVE).to(torch.int32)
    else:
        pos = torch.full((M,), LIVE, dtype=torch.int32, device=dev)
        sid = torch.arange(M, dtype=torch.int32, device=dev)
    kc = torch.zeros(SEQS, HKV, T, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    gq = (1.0 + 0.3 * torch.randn(D)).to(dev)
    gk = (1.0 + 0.3 * torch.randn(D)).to(dev)
    modes = {
        "qknorm_rope_kv": lambda i: B.qknorm_rope_kv(bufs[i % copies], k_off, v_off, gq, gk, 1e-6, cos, sin, pos, sid, kc, vc, H, HKV,
                                                     D, T),
        "rope_kv_gqa": lambda i: B.rope_kv_gqa(bufs[i % copies], k_off, v_off, cos, sin, pos, sid, kc, vc, H, HKV, D, T),
    }
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
        rec = {"kernel": m, "rows": M, "n_heads": H, "n_kv_heads": HKV, "us_median": round(us, 2), "us_min": round(min(ts), 2),
               "bytes_moved": moved, "eff_tb_s": round(moved / us / 1e6, 3), "buffer_copies_rotated": copies,
               "streams_from_hbm": bool(copies * moved >= 2 * L3_BYTES)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    ratio = recs[0]["us_median"] / recs[1]["us_median"]
    print(f"rows {M}: qknorm_rope_kv / rope_kv_gqa = {ratio:.3f}", flush=True)
    del bufs
    torch.cuda.empty_cache()
    return recs, round(ratio, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "head_dim": D, "cache_len": T, "legs": [], "ratio_qknorm_over_rope": {}}
    for M in (1, SEQS, SEQS * LIVE):
        recs, ratio = leg(M, args.rounds, args.reps)
        res["legs"] += recs
        res["ratio_qknorm_over_rope"][str(M)] = ratio
    print(json.dumps(res["ratio_qknorm_over_rope"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
