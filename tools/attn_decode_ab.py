"""Time the seven decode-attention entry points — every entry point of csrc/attn_decode.hip — for two or more builds
(name=path ...), interleaved, on seeded inputs, and compare what they write bit for bit: the output, and for the RoPE-fused forms
the caches and scale planes (each build appends to a copy of its own).  The masked form runs under a mask that blocks some
segments for every head and all of them for none.  Loading one build under two names shows the spread that a difference between
builds has to exceed.
usage: python tools/attn_decode_ab.py base=lib/libicl_hip_base.so base2=lib/libicl_hip_base2.so new=lib/libicl_hip.so"""
import ctypes, functools, math, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icl_speech_text_llm_amd.runtime.binding import _SIGNATURES

L, LIVE, ROUNDS, REPS = 448, 386, 7, 50
dev = "cuda"
bf16 = lambda *shape: (torch.randn(*shape, device=dev) * 0.5).to(torch.bfloat16)


def cache(n, H, D, fp8):
    """K and V rows [n, H, L, D] and their scale planes: bf16 and none, or e4m3fn codes (finite, |x| < 32) and 2^-8 .. 2^-5."""
    if not fp8:
        return [bf16(n, H, L, D), bf16(n, H, L, D)], []
    codes = lambda: (torch.randint(0, 0x60, (n, H, L, D), device=dev) | torch.randint(0, 2, (n, H, L, D), device=dev) << 7).to(torch.uint8)
    scales = lambda: torch.exp2(torch.randint(-8, -4, (n, H, L), device=dev).float())
    return [codes(), codes()], [scales(), scales()]


def plain(n, H, Hkv, D, fp8=False, gqa=False):
    q, (kv, sc) = bf16(n, H * D), cache(n, Hkv, D, fp8)
    lens = torch.full((n,), LIVE, dtype=torch.int32, device=dev)

    def build(stream):
        o = torch.empty(n, H * D, dtype=torch.bfloat16, device=dev)
        heads = [H, Hkv] if gqa else [H]
        return [q, H * D, *kv, *sc, o, H * D, lens, n, *heads, D, L, D ** -0.5, stream], [o]
    return build


def fused(n, H, Hkv, D, fp8=False):
    """The step's q | k | v rows; every sequence appends position LIVE - 1 of a cache that holds LIVE - 1 keys."""
    qkv, (kv, sc) = bf16(n, 3 * H * D), cache(n, H, D, fp8)
    ang = torch.arange(L, device=dev, dtype=torch.float64)[:, None] * 10000.0 ** (-torch.arange(D // 2, device=dev, dtype=torch.float64) * 2 / D)
    cos, sin = ang.cos().float(), ang.sin().float()
    lens = torch.full((n,), LIVE, dtype=torch.int32, device=dev)
    pos = lens - 1

    def build(stream):
        o = torch.empty(n, H * D, dtype=torch.bfloat16, device=dev)
        own = [t.clone() for t in kv + sc]
        return [qkv, 3 * H * D, H * D, 2 * H * D, cos, sin, pos, None, *own, o, H * D, lens, n, H, D, L, D ** -0.5, stream], [o] + own
    return build


def masked(n, H, Hkv, D):
    """n list entries over n cache sequences, in reverse order; 64-key segments, every (entry, head) blocks a random set of the
    segments 1 .. 6 and never segment 0, so no head is left without a key."""
    q, (kv, _) = bf16(n, H * D), cache(n, Hkv, D, False)
    lens = torch.full((n,), LIVE, dtype=torch.int32, device=dev)
    seg = (torch.arange(L, device=dev) // 64).to(torch.uint8).repeat(n, 1)
    blocked = (torch.randint(0, 64, (n, H), device=dev) << 1).to(torch.int32)
    rows = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=dev)

    def build(stream):
        o = torch.zeros(n, H * D, dtype=torch.bfloat16, device=dev)
        return [q, H * D, *kv, o, H * D, lens, seg, L, blocked, rows, rows, n, H, Hkv, D, L, D ** -0.5, stream], [o]
    return build


ENTRIES = [("icl_attn_decode_bf16", plain), ("icl_attn_decode_bf16_epl16", plain), ("icl_attn_decode_fp8", functools.partial(plain, fp8=True)),
           ("icl_attn_decode_rope_bf16", fused), ("icl_attn_decode_rope_fp8", functools.partial(fused, fp8=True))]
MHA = [(n, 32, 32, 128) for n in (1, 16, 256)] + [(n, 16, 16, 64) for n in (1, 256)]           # n_seqs, heads, K/V heads, head_dim
GQA = [(n, H, Hkv, 128) for H, Hkv in ((32, 16), (32, 8), (28, 4), (32, 4)) for n in (1, 256)]
MASKED = [(n, 32, Hkv, 128) for Hkv in (32, 8) for n in (1, 256)]                              # n = list entries
CASES = ([(e, b, s) for e, b in ENTRIES for s in MHA] + [("icl_attn_decode_gqa_bf16", functools.partial(plain, gqa=True), s) for s in GQA] +
         [("icl_attn_decode_masked_bf16", masked, s) for s in MASKED])

libs = [(name, ctypes.CDLL(os.path.abspath(path))) for name, path in (spec.split("=", 1) for spec in sys.argv[1:])]
bits = lambda t: t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])
ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
for entry, builder, (n, H, Hkv, D) in CASES:
    torch.manual_seed(n)
    build = builder(n, H, Hkv, D)
    calls, written, times = [], [], {name: [] for name, _ in libs}
    for name, lib in libs:
        fn = getattr(lib, entry)
        fn.restype, fn.argtypes = _SIGNATURES[entry]
        args, outs = build(torch.cuda.current_stream().cuda_stream)
        calls.append(functools.partial(fn, *map(ptr, args)))
        written.append((args, outs))          # args: keeps the tensors behind the pointers alive
        for _ in range(5):
            assert calls[-1]() == 0, entry
    for _ in range(ROUNDS):
        for (name, _), call in zip(libs, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                call()
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / REPS * 1e3)
    same = all(torch.equal(bits(a), bits(b)) for _, outs in written[1:] for a, b in zip(written[0][1], outs))
    o = written[0][1][0]
    live = math.isfinite(float(o.float().abs().sum())) and bool(o.any())       # equal zeros or NaNs would say nothing
    print(f"{entry:28s} D={D:3d} heads={H}/{Hkv} B={n:3d}  " + "  ".join(f"{k}: {statistics.median(t):7.1f} us" for k, t in times.items()) +
          f"  bit-equal={same}" + ("" if live else "  (degenerate output)"), flush=True)
    del build, calls, written
    torch.cuda.empty_cache()
