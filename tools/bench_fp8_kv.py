"""FP8 KV cache vs bf16 on one box, interleaved (the tools/ab_bench_b1.sh manner).

  1. decode attention per launch at the Llama-2-7B shape (32 heads x 128, cache length 448, bench.py's ~386 live positions):
     icl_attn_decode_bf16 vs icl_attn_decode_fp8, and the RoPE-fused forms, at 256 sequences and at 1; median us and the
     effective TB/s of the cache bytes each kernel reads;
  2. the prefill quantize-append pass (icl_kv_append_fp8) per layer at a 128-sequence prefill chunk of bench.py's prompts;
  3. the C2 workload (SALMONN 7B dims, bench.py's synthetic utterances and prompt layout: speech encoder, prefill + 10 greedy
     tokens) at micro-batch 256 and at batch 1: one runtime, the cache dtype alternating between rounds.  Decode ms per step =
     (10-token call - 1-token call) / 9; utt/s end to end (encoder + generate) and of the LLM stage alone.
  Also the workspace bytes of each mode at micro-batch 256, and the largest micro-batch whose workspace would fit the device
  (the workspace scaled linearly from 256, next to the weights).

    python tools/bench_fp8_kv.py [--rounds 3] [--out profiles/r05_fp8_kv.json]
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

H, D, T = 32, 128, 448
LIVE = 386                      # bench.py's prompt (~376 positions) plus the 10 generated tokens, rounded


def _time(fn, reps, rounds_out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        fn(i)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    rounds_out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]


def attention_leg(rounds: int, reps: int):
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    out = []
    for n in (256, 1):
        copies = 2 if n == 256 else 128                     # every call streams its cache from HBM (> the 256 MiB Infinity Cache)
        kc = [(torch.randn(n, H, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
        vc = [(torch.randn(n, H, T, D, device=dev) * 0.5).to(torch.bfloat16) for _ in range(copies)]
        k8 = [torch.randint(0, 120, (n, H, T, D), dtype=torch.uint8, device=dev) for _ in range(copies)]
        v8 = [torch.randint(0, 120, (n, H, T, D), dtype=torch.uint8, device=dev) for _ in range(copies)]
        ks = [torch.full((n, H, T), 2.0 ** -6, device=dev) for _ in range(copies)]
        qkv = (torch.randn(n, 3 * H * D, device=dev) * 0.5).to(torch.bfloat16)
        o = torch.empty(n, H * D, dtype=torch.bfloat16, device=dev)
        lens = torch.full((n,), LIVE, dtype=torch.int32, device=dev)
        pos = lens - 1
        sid = torch.arange(n, dtype=torch.int32, device=dev)
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
        f = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
        cos, sin = f.cos().float().to(dev).contiguous(), f.sin().float().to(dev).contiguous()
        hd = H * D
        modes = {
            "bf16": lambda i: B.attn_decode(qkv[:, :hd], kc[i % copies], vc[i % copies], o, lens, H, D, T, D ** -0.5),
            "fp8": lambda i: B.attn_decode_fp8(qkv[:, :hd], k8[i % copies], v8[i % copies], ks[i % copies], ks[i % copies], o, lens,
                                               H, D, T, D ** -0.5),
            "bf16_rope_fused": lambda i: B.attn_decode_rope(qkv, hd, 2 * hd, cos, sin, pos, sid, kc[i % copies], vc[i % copies], o,
                                                            lens, H, D, T, D ** -0.5),
            "fp8_rope_fused": lambda i: B.attn_decode_rope_fp8(qkv, hd, 2 * hd, cos, sin, pos, sid, k8[i % copies], v8[i % copies],
                                                               ks[i % copies], ks[i % copies], o, lens, H, D, T, D ** -0.5),
        }
        times = {m: [] for m in modes}
        for fn in modes.values():
            for i in range(copies):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for m, fn in modes.items():
                _time(fn, reps, times[m])
        for m, ts in times.items():
            us = statistics.median(ts)
            nbytes = n * H * LIVE * D * 2 * (1 if m.startswith("fp8") else 2) + (n * H * LIVE * 8 if m.startswith("fp8") else 0)
            rec = {"leg": "attn_decode", "n_seqs": n, "live_positions": LIVE, "mode": m, "us_median": round(us, 2),
                   "us_min": round(min(ts), 2), "cache_bytes_read": nbytes, "eff_tb_s": round(nbytes / us / 1e6, 2)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del kc, vc, k8, v8, ks
        torch.cuda.empty_cache()
    return out


def append_leg(rounds: int, reps: int):
    """icl_kv_append_fp8 over one prefill chunk (128 sequences x bench.py's prompt length) of one layer."""
    import bench
    import icl_speech_text_llm_amd.runtime.binding as B
    dev = torch.device("cuda")
    S = bench.S_TEXT + bench.N_AUDIO_TOK + 2                 # an upper bound of bench.py's prompt length (text + speech + tags)
    n = 128
    M = n * S
    qkv = (torch.randn(M, 3 * H * D, device=dev) * 0.5).to(torch.bfloat16)
    pos = torch.arange(S, dtype=torch.int32, device=dev).repeat(n)
    sid = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(S)
    k8 = torch.empty(n, H, T, D, dtype=torch.uint8, device=dev)
    v8 = torch.empty_like(k8)
    ks = torch.empty(n, H, T, device=dev)
    vs = torch.empty_like(ks)
    ts = []
    fn = lambda i: B.kv_append_fp8(qkv, H * D, 2 * H * D, pos, sid, k8, v8, ks, vs, H, D, T)
    fn(0)
    torch.cuda.synchronize()
    for _ in range(rounds):
        _time(fn, reps, ts)
    us = statistics.median(ts)
    nbytes = M * 2 * H * D * 2 + M * 2 * H * (D + 4)
    rec = {"leg": "prefill_append", "rows": M, "sequences": n, "us_per_layer_median": round(us, 2), "us_min": round(min(ts), 2),
           "bytes": nbytes, "eff_tb_s": round(nbytes / us / 1e6, 2)}
    print(json.dumps(rec), flush=True)
    return rec


def llm_leg(rounds: int):
    import bench
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    dev = torch.device("cuda")
    cfg = SalmonnCfg.llama2_7b()
    sd = synth.salmonn_state(cfg, seed=0, device=dev, dtype=torch.bfloat16)
    rt = SalmonnRuntime(cfg, sd, device=dev, consume=True)
    del sd
    torch.cuda.synchronize()
    res = {}
    for n in (256, 1):
        wav, ids = bench.synth_utterances(0, n, cfg.llama.vocab)
        wav = torch.from_numpy(wav).to(dev)
        prompts = bench.build_prompts(ids)

        def encode():
            return rt.encode_speech(wav, [wav.shape[1]] * n)

        def call(k, speech):
            return rt.generate(prompts, speech, max_new_tokens=k, suppress_eos=True)
        speech = encode()
        toks = {}
        for mode in ("bf16", "fp8"):                         # warm-up: buffers sized, decode graphs captured
            rt.kv_dtype = mode
            for _ in range(2):
                toks[mode] = call(bench.NEW_TOKENS, speech).tokens
                call(1, speech)
            torch.cuda.synchronize()
        t = {m: {"encode": [], "one": [], "full": []} for m in ("bf16", "fp8")}
        for r in range(rounds):
            for mode in ("bf16", "fp8"):
                rt.kv_dtype = mode
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                speech = encode()                            # the speech encoder: the same work in both modes
                torch.cuda.synchronize()
                t[mode]["encode"].append((time.perf_counter() - t0) * 1e3)
                for key, k in (("one", 1), ("full", bench.NEW_TOKENS)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(k, speech)
                    torch.cuda.synchronize()
                    t[mode][key].append((time.perf_counter() - t0) * 1e3)
                rec = {"leg": "c2", "n": n, "round": r, "mode": mode, "ms_encode": round(t[mode]["encode"][-1], 2),
                       "ms_prefill_1tok": round(t[mode]["one"][-1], 2), "ms_10tok": round(t[mode]["full"][-1], 2)}
                print(json.dumps(rec), flush=True)
        summ = {}
        for mode in ("bf16", "fp8"):
            enc, one, full = (statistics.median(t[mode][k]) for k in ("encode", "one", "full"))
            summ[mode] = {"ms_encode": round(enc, 2), "ms_prefill_plus_first_token": round(one, 2), "ms_10_tokens": round(full, 2),
                          "decode_ms_per_step": round((full - one) / (bench.NEW_TOKENS - 1), 2),
                          "llm_utt_per_s": round(n / full * 1e3, 2), "end_to_end_utt_per_s": round(n / (enc + full) * 1e3, 2),
                          "raw_ms_10_tokens": [round(x, 2) for x in t[mode]["full"]]}
        summ["tokens_equal_to_bf16"] = bool(torch.equal(toks["bf16"], toks["fp8"]))
        summ["token_agreement"] = round(float((toks["bf16"] == toks["fp8"]).float().mean()), 4)
        if n == 256:
            total = torch.cuda.get_device_properties(0).total_memory
            cache_bf16 = cfg.llama.n_layers * n * H * T * D * 2 * 2
            cache_fp8 = cfg.llama.n_layers * n * H * T * (D + 4) * 2
            for mode, cache in (("bf16", cache_bf16), ("fp8", cache_fp8)):
                rt.kv_dtype = mode
                rt.ws.clear()
                call(bench.NEW_TOKENS, encode())
                torch.cuda.synchronize()
                wsb = rt.ws.nbytes()
                fixed = torch.cuda.memory_allocated() - wsb       # weights and everything that is not the workspace
                summ[mode]["workspace_bytes_mb256"] = wsb
                summ[mode]["kv_cache_bytes_mb256"] = cache
                summ[mode]["max_micro_batch_fits_est"] = int((0.95 * total - fixed) / (wsb / n))
            rt.ws.clear()
        res[f"n{n}"] = summ
        print(json.dumps({"leg": "c2_summary", "n": n, **{k: v for k, v in summ.items()}}), flush=True)
        del wav, speech
    return res


def summarize(res):
    a = {(r["n_seqs"], r["mode"]): r["us_median"] for r in res["attn_decode"]}
    out = {"attn_decode_us_256_rows": {m: a[(256, m)] for m in ("bf16", "fp8", "bf16_rope_fused", "fp8_rope_fused")},
           "attn_decode_ratio_256_rows": round(a[(256, "fp8")] / a[(256, "bf16")], 3),
           "attn_decode_ratio_256_rows_fused": round(a[(256, "fp8_rope_fused")] / a[(256, "bf16_rope_fused")], 3),
           "prefill_append_ms_per_mb256_step": round(res["prefill_append"]["us_per_layer_median"] * 32 * 2 / 1e3, 2)}
    c2 = res.get("c2")
    if c2:
        for n in ("n256", "n1"):
            for key in ("decode_ms_per_step", "ms_prefill_plus_first_token", "end_to_end_utt_per_s", "llm_utt_per_s"):
                out[f"{key}_{n}"] = {m: c2[n][m][key] for m in ("bf16", "fp8")}
        out["max_micro_batch_fits_est"] = {m: c2["n256"][m]["max_micro_batch_fits_est"] for m in ("bf16", "fp8")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip-c2", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    res = {"command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", "")}
    res["attn_decode"] = attention_leg(args.rounds, args.reps)
    res["prefill_append"] = append_leg(args.rounds, args.reps)
    if not args.skip_c2:
        res["c2"] = llm_leg(args.rounds)
    res["summary"] = summarize(res)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
