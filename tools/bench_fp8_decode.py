"""FP8 weight mode vs bf16 at the batch-1 operating point, on one box, interleaved (the tools/ab_bench_b1.sh manner).

  1. per decoder GEMM of Llama-2-7B, at 1 and 8 rows: bf16 tile 6 (decode-packed W') vs the fp8-weight kernel (icl_gemm_fp8w),
     median us over rotating weight copies (more bytes than the 256 MiB Infinity Cache, so every call streams from HBM) and the
     effective TB/s of the bytes each kernel actually reads (weights + activations);
  2. per-utterance ms of the C2 workload (bench.py's synthetic utterances, 7B, encode + prefill + 10 greedy tokens) at batch 1,
     SalmonnRuntime built once in each mode, rounds alternating between the two.

    python tools/bench_fp8_decode.py [--rounds 3] [--utts 10] [--out profiles/r05_fp8_decode.json]
Prints one line per measurement and a JSON summary (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"qkv": (3 * 4096, 4096 + 64), "o": (4096, 4096), "gu": (2 * 11008, 4096), "down": (4096, 11008)}


def gemm_leg(rounds: int, reps: int):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    out = []
    for name, (N, K) in SHAPES.items():
        copies = max(2, -(-600 * 2**20 // (N * K * 2)))          # > 256 MiB of bf16 weights per rotation
        packs = []
        for c in range(copies):
            w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
            q, s, wd = B.pack_fp8_weights(w)
            del w
            packs.append((B.pack_decode_weights(wd), q, s))
            del wd
        for M in (1, 8):
            a = torch.randn(M, K, device=dev).to(torch.bfloat16)
            sw = name == "gu"
            o = torch.empty(M, N // 2 if sw else N, dtype=torch.bfloat16, device=dev)
            times = {"bf16_tile6": [], "fp8w": []}

            def run(mode, i):
                dp, q, s = packs[i % copies]
                if mode == "bf16_tile6":
                    B.gemm(a, dp, o, swiglu=sw, tile=6, N=N, K=K)
                else:
                    B.gemm(a, q, o, swiglu=sw, w_scale=s, N=N, K=K)
            for mode in times:                     # warm-up
                for i in range(copies):
                    run(mode, i)
            torch.cuda.synchronize()
            for r in range(rounds):
                for mode in times:
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
                    for i in range(reps):
                        ev[2 * i].record()
                        run(mode, i)
                        ev[2 * i + 1].record()
                    torch.cuda.synchronize()
                    times[mode] += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]
            for mode, ts in times.items():
                us = statistics.median(ts)
                wbytes = N * K * (2 if mode == "bf16_tile6" else 1)
                rec = {"gemm": name, "N": N, "K": K, "M": M, "mode": mode, "us_median": round(us, 2),
                       "us_min": round(min(ts), 2), "weight_bytes": wbytes,
                       "eff_tb_s": round((wbytes + M * K * 2) / us / 1e6, 2)}      # weights + activations, once
                print(json.dumps(rec), flush=True)
                out.append(rec)
        del packs
        torch.cuda.empty_cache()
    return out


def utterance_leg(rounds: int, utts: int):
    import bench
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    dev = torch.device("cuda")
    cfg = SalmonnCfg.llama2_7b()
    sd = synth.salmonn_state(cfg, seed=0, device=dev, dtype=torch.bfloat16)
    rts = {mode: SalmonnRuntime(cfg, dict(sd), device=dev, llm_weight_dtype=mode) for mode in ("bf16", "fp8")}
    del sd
    torch.cuda.synchronize()
    inputs = []
    for i in range(utts):
        w, ids = bench.synth_utterances(i, 1, cfg.llama.vocab)
        inputs.append((torch.from_numpy(w).to(dev), bench.build_prompts(ids)))

    def one(rt, i):
        wav, prompts = inputs[i]
        speech = rt.encode_speech(wav, [480000])
        return rt.generate(prompts, speech, max_new_tokens=bench.NEW_TOKENS, suppress_eos=True, want_first_logits=True)
    first = {}
    for mode, rt in rts.items():                  # two passes: the second captures the decode graph
        for _ in range(2):
            first[mode] = one(rt, 0).tokens[0].tolist()
        torch.cuda.synchronize()
    ms = {m: [] for m in rts}
    for r in range(rounds):
        for mode, rt in rts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(utts):
                one(rt, i)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) / utts * 1e3)
            print(json.dumps({"round": r, "mode": mode, "ms_per_utterance": round(ms[mode][-1], 2)}), flush=True)
    return {"ms_per_utterance": {m: [round(x, 2) for x in v] for m, v in ms.items()},
            "median": {m: round(statistics.median(v), 2) for m, v in ms.items()},
            "first_utterance_tokens": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--utts", type=int, default=10)
    ap.add_argument("--skip-gemm", action="store_true")
    ap.add_argument("--skip-utterance", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not args.skip_gemm:
        res["gemm"] = gemm_leg(args.rounds, args.reps)
    if not args.skip_utterance:
        res["batch1_c2"] = utterance_leg(args.rounds, args.utts)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
