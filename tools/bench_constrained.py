"""Constrained decode tail vs the plain one on one box, one process, interleaved rounds.

  1. per launch: icl_argmax_eos, icl_argmax_fsm with every row free, icl_argmax_fsm with every row constrained (rows spread over
     the start states of all typed tasks, byte-tokenizer automaton), at B = 256, V = 32001 and at B = 64, V = 156032; median us
     over rounds x reps launches, the logits rotating over 4 buffers;
  2. a 256-row generate() of 10 tokens with and without a constraint on a MINIATURE decoder (2 layers, hidden 256) with the full
     32001-id vocabulary: the tail's share of a step is far larger there than in a 7B step, so the ratio bounds the end-to-end
     difference of a real model from above.
Every GPU step runs under its own time limit (the process exits with a traceback if a step overruns it).

    python tools/bench_constrained.py [--rounds 5] [--reps 50] [--out profiles/r06_constrained.json]
Prints one line per measurement and a JSON summary (also written to --out)."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time
from contextlib import contextmanager

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextmanager
def limit(seconds: int):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _automaton(vocab: int):
    from icl_speech_text_llm_amd.data.task_configs import DatasetType
    from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
    from icl_speech_text_llm_amd.utils.tokenization import ByteTokenizer
    return build_label_automaton(ByteTokenizer(vocab), list(DatasetType))


def _time(fn, reps, out):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        fn(i)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]


def kernel_leg(B: int, V: int, rounds: int, reps: int):
    import icl_speech_text_llm_amd.runtime.binding as Bd
    dev = torch.device("cuda")
    a = _automaton(V)
    tables = a.upload(dev)
    starts = [s for s in a.starts.values() if s >= 0]
    lg = [torch.randn(B, V, device=dev) * 3 for _ in range(4)]
    st_con = torch.tensor([starts[b % len(starts)] for b in range(B)], dtype=torch.int32, device=dev)
    st_free = torch.full((B,), -1, dtype=torch.int32, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev)
    toks = torch.zeros(B, 10, dtype=torch.int32, device=dev)
    lps = torch.zeros(B, 10, dtype=torch.float32, device=dev)
    nxt = torch.zeros(B, dtype=torch.int32, device=dev)

    # no EOS id (-1), so no row finishes and every launch does its full work.  A constrained row moves
    # along its label, so the row states restart before every launch of the fsm modes, ahead of the start event
    def fsm(src):
        def go(out):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
            for i in range(reps):
                st.copy_(src)
                ev[2 * i].record()
                Bd.argmax_fsm(lg[i % 4], tables, st, 10, -1, V - 1, fin, toks, 0, nxt, out_logprob=lps)
                ev[2 * i + 1].record()
            torch.cuda.synchronize()
            out += [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps)]
        return go

    def eos(out):
        _time(lambda i: Bd.argmax_eos(lg[i % 4], -1, V - 1, fin, toks, 0, nxt), reps, out)

    modes = {"argmax_eos": eos, "argmax_fsm_free": fsm(st_free), "argmax_fsm_constrained": fsm(st_con)}
    times = {m: [] for m in modes}
    with limit(120):
        for fn in modes.values():
            fn([])                                            # warm-up
        for _ in range(rounds):
            for m, fn in modes.items():
                fn(times[m])
        assert not bool(fin.any())
    out = {}
    for m, ts in times.items():
        out[m] = {"median_us": round(statistics.median(ts), 2), "p10_us": round(float(np.percentile(ts, 10)), 2),
                  "p90_us": round(float(np.percentile(ts, 90)), 2), "launches": len(ts)}
        print(f"B={B} V={V} {m}: median {out[m]['median_us']} us (p10 {out[m]['p10_us']}, p90 {out[m]['p90_us']}, {len(ts)} launches)")
    return {"B": B, "V": V, "automaton_states": a.n_states, "automaton_edges": a.n_edges, "modes": out}


def generate_leg(rounds: int):
    from icl_speech_text_llm_amd.runtime import synth
    from icl_speech_text_llm_amd.runtime.config import SalmonnCfg
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    V, Bn, T = 32001, 256, 10
    cfg = SalmonnCfg.tiny(use_beats=False, lora=False, vocab=V)
    with limit(300):
        sd = synth.salmonn_state(cfg, seed=3, jitter=True, parts=("llama",))
        rt = SalmonnRuntime(cfg, dict(sd), device="cuda", parts=("llama",))
    a = _automaton(V)
    starts = [s for s in a.starts.values() if s >= 0 and a.min_tokens(s) <= T]
    cons = (a, [starts[b % len(starts)] for b in range(Bn)])
    prompts = [[np.random.default_rng(b).integers(3, V - 1, 64).tolist()] for b in range(Bn)]
    eos, pad = cfg.llama.eos_id, cfg.llama.pad_id
    modes = {"unconstrained": None, "constrained": cons}
    times = {m: [] for m in modes}

    def run(c):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = rt.generate(prompts, None, max_new_tokens=T, eos_id=eos, pad_id=pad, constraint=c)     # ends in the D2H of the tokens
        return (time.perf_counter() - t0) * 1e3, res

    with limit(300):
        for c in modes.values():
            for _ in range(3):                                # eager, capture, replay
                run(c)
        for _ in range(rounds):
            for m, c in modes.items():
                for _ in range(5):
                    times[m].append(run(c)[0])
    out = {m: {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "calls": len(ts)} for m, ts in times.items()}
    for m, o in out.items():
        print(f"generate 256 rows x {T} tokens (miniature decoder, V={V}) {m}: median {o['median_ms']} ms (min {o['min_ms']}, {o['calls']} calls)")
    return {"rows": Bn, "new_tokens": T, "vocab": V, "decoder": "2 layers, hidden 256", "modes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    summary = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps,
               "kernel": [kernel_leg(256, 32001, args.rounds, args.reps), kernel_leg(64, 156032, args.rounds, args.reps)],
               "generate": generate_leg(args.rounds)}
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
