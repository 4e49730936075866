"""Time the RoPE + KV-append entry points of csrc/rope_kv.hip for two or more builds (name=path ...), interleaved, on seeded
inputs, and compare what they write bit for bit: the qkv buffers, the caches and the scale planes (every build works on copies
of its own and runs the same launches, so the states it leaves are comparable).  Loading one build under two names (two copies
of the file) shows the spread that a difference between builds has to exceed: per entry point, the largest relative gap between
base and base2 over its shapes; a later build regresses at a shape where (build - base) / base exceeds it.
usage: python tools/rope_kv_ab.py base=lib/libicl_hip_base.so base2=lib/libicl_hip_base2.so new=lib/libicl_hip.so [entry point ...]
Run it under a time limit of its own (``timeout -k 10 600 python tools/rope_kv_ab.py ...``)."""
import ctypes, functools, math, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from icl_speech_text_llm_amd.runtime.binding import _SIGNATURES

L, POS, SEQS, ROUNDS, REPS = 448, 385, 256, 15, 50
L3_BYTES, MAX_COPIES = 256 << 20, 64
CHUNK = (128, bench.S_TEXT + bench.N_AUDIO_TOK + 2)     # the prefill chunk of tools/bench_fp8_kv.py's append leg: sequences x rows
dev = "cuda"


def inputs(entry, M, H, Hkv, D):
    """Seeded inputs of one case, and build(stream) -> (argument list, tensors written) on fresh copies of what a launch writes.
    M rows: one new position POS per sequence, or whole prompts (M = sequences x rows: positions 0 .. rows - 1 of each)."""
    fp8, norm = entry.endswith("fp8"), "qknorm" in entry
    width, k_off, v_off = (H + 2 * Hkv) * D, H * D, (H + Hkv) * D
    if isinstance(M, tuple):
        n, rows = M
        pos = torch.arange(rows, dtype=torch.int32, device=dev).repeat(n)
        sid = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(rows)
        M = n * rows
    else:
        n = SEQS
        pos = torch.full((M,), POS, dtype=torch.int32, device=dev)
        sid = torch.arange(M, dtype=torch.int32, device=dev)
    moved = M * width * 2 * 2                               # an upper bound of the bytes a launch moves: the row read and written
    copies = max(2, min(MAX_COPIES, -(-2 * L3_BYTES // moved)))          # the large legs rotate through > the Infinity Cache
    qkv = (torch.randn(M, width, device=dev) * 0.5).to(torch.bfloat16)
    ang = torch.arange(L, device=dev, dtype=torch.float64)[:, None] * 10000.0 ** (-torch.arange(D // 2, device=dev, dtype=torch.float64) * 2 / D)
    cos, sin = ang.cos().float(), ang.sin().float()
    gq, gk = 1.0 + 0.3 * torch.randn(D, device=dev), 1.0 + 0.3 * torch.randn(D, device=dev)

    def build(stream):
        bufs = [qkv.clone() for _ in range(copies)]
        if fp8:
            cache = [torch.full((n, Hkv, L, D), 0x55, dtype=torch.uint8, device=dev) for _ in range(2)]
            cache += [torch.full((n, Hkv, L), -1.0, device=dev) for _ in range(2)]
        else:
            cache = [torch.zeros(n, Hkv, L, D, dtype=torch.bfloat16, device=dev) for _ in range(2)]
        head = [[b, width, k_off, v_off] for b in bufs]
        tail = {"icl_rope_kv_bf16": [cos, sin, pos, sid, *cache, M, H, D, L, stream],
                "icl_rope_kv_gqa_bf16": [cos, sin, pos, sid, *cache, M, H, Hkv, D, L, stream],
                "icl_qknorm_rope_kv_bf16": [gq, gk, 1e-6, cos, sin, pos, sid, *cache, M, H, Hkv, D, L, stream],
                "icl_rope_kv_fp8": [cos, sin, pos, sid, *cache, M, H, D, L, stream],
                "icl_kv_append_fp8": [pos, sid, *cache, M, H, D, L, stream]}[entry]
        return [h + tail for h in head], bufs + cache
    return build


CASES = ([("icl_qknorm_rope_kv_bf16", M, 32, 8, 128) for M in (1, SEQS, (SEQS, POS))] +       # the legs of tools/bench_qknorm.py
         [("icl_qknorm_rope_kv_bf16", M, 16, 16, 64) for M in (1, SEQS)] +
         [("icl_rope_kv_fp8", M, 32, 32, 128) for M in (1, 8, SEQS)] +                        # decode runs it at 8 rows and below
         [("icl_kv_append_fp8", M, 32, 32, 128) for M in (CHUNK, SEQS)] +
         [("icl_rope_kv_bf16", M, 32, 32, 128) for M in (1, 128)])                            # a control: moved, not changed

libs = [(name, ctypes.CDLL(os.path.abspath(path))) for name, path in (spec.split("=", 1) for spec in sys.argv[1:] if "=" in spec)]
only = [a for a in sys.argv[1:] if "=" not in a]            # entry-point names: time these alone
bits = lambda t: t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])
ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
medians = {}
for entry, M, H, Hkv, D in [c for c in CASES if not only or c[0] in only]:
    torch.manual_seed(H + D)
    build = inputs(entry, M, H, Hkv, D)
    calls, written, times = [], [], {name: [] for name, _ in libs}
    for name, lib in libs:
        fn = getattr(lib, entry)
        fn.restype, fn.argtypes = _SIGNATURES[entry]
        arglists, outs = build(torch.cuda.current_stream().cuda_stream)
        calls.append([functools.partial(fn, *map(ptr, args)) for args in arglists])
        written.append((arglists, outs))      # arglists: keeps the tensors behind the pointers alive
        for call in calls[-1]:
            assert call() == 0, entry
    for _ in range(ROUNDS):
        for (name, _), cs in zip(libs, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(REPS):
                cs[i % len(cs)]()
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / REPS * 1e3)
    same = all(torch.equal(bits(a), bits(b)) for _, outs in written[1:] for a, b in zip(written[0][1], outs))
    live = all(math.isfinite(float(o.float().abs().sum())) and bool(o.any()) for o in written[0][1])   # equal zeros or NaNs would say nothing
    rows = f"{M[0]}x{M[1]}" if isinstance(M, tuple) else str(M)
    med = {k: statistics.median(t) for k, t in times.items()}
    medians.setdefault(entry, []).append((f"D={D} heads={H}/{Hkv} M={rows}", med))
    print(f"{entry:24s} D={D:3d} heads={H}/{Hkv} M={rows:>7s} x{len(calls[0]):2d} buffers  " +
          "  ".join(f"{k}: {v:7.1f} us" for k, v in med.items()) + f"  bit-equal={same}" + ("" if live else "  (degenerate output)"), flush=True)
    del build, calls, written
    torch.cuda.empty_cache()

if {"base", "base2"} <= {name for name, _ in libs}:
    for entry, shapes in medians.items():
        spread = max(abs(m["base2"] - m["base"]) / m["base"] for _, m in shapes)
        over = [f"{k} {shape} {100 * (m[k] - m['base']) / m['base']:+.2f} %" for shape, m in shapes for k in m
                if k not in ("base", "base2") and (m[k] - m["base"]) / m["base"] > spread]
        print(f"{entry}: spread {100 * spread:.2f} %; over it: {'; '.join(over) if over else 'nothing'}", flush=True)
