"""Far-offset tests: offsets are 64-bit from the binding to the last store (`-m gpu`; every call goes through runtime/binding.py).

Every other GPU test uses operands of a few megabytes, so address arithmetic that only goes wrong when an offset no longer fits
in 32 bits passes all of them.  Here every entry point below runs on operands that are views into ONE arena of 2^34 + 2^28 bytes
(16.25 GiB; an f32 operand needs element offsets >= 2^32, which is 16 GiB), allocated once per module and freed at teardown, with
at least one operand addressed at a true offset of >= 2^32 elements of its own type from the pointer the kernel receives.  Only
small windows of the arena are ever filled or compared.  tests/far_layout.py places the operands (the three forms — stride,
index, grid-walk — are described there) and tests/test_far_layout.py shows on the CPU that no 32-bit narrowing of any address
leaves the arena, that each lands in a window compared here, and that the assertions below reject each.

Per case: the windows are filled (inputs from a seeded generator, outputs NaN / 0xFF, a 64 KiB margin of 0xA5 bytes around every
region), the entry point runs on the far views, then again on a compact twin (same values in small tensors, same pointer
alignment, same ld % 8, same sequence count: the launcher picks the same kernel), and
  1. the far outputs are bit-identical to the twin's (no tolerance: address arithmetic does not change arithmetic),
  2. the twin is within the project's existing fp64 bound of that kernel (tests/fp64_bounds.py, oracle/attention.py,
     tests/qknorm_ref.py; the fp8 forms by their bit-identity anchor, ref_q of tests/fp8_ref.py),
  3. every compared window outside the expected outputs is bit-equal to its pre-launch clone (margins, the near window where a
     truncated write would land, inputs).

Covered, by form (stride / index / grid-walk as in tests/far_layout.py):
  norms         rmsnorm, layernorm (with res + out2 and without): x, res, y, y2 far (stride); N = 1280 f32 -> bf16 without residual
                (norm8_kernel) and N = 4096 / the residual forms (norm_kernel)
  RoPE + append rope_kv, rope_kv_gqa, qknorm_rope_kv, rope_kv_fp8, kv_append_fp8: qkv rows far (stride), cache rows far (index
                through seq_ids); *_many_ids: compact qkv and several near and far ids, the fp8 byte planes at 2^32 k + d for
                k = 1, 2, 3
  glue          gather_rows f32 / bf16 (src by idx, out by ld_out), axpby_cast (all three operands, both dtypes),
                embed_gather_interleave (table by far token ids, speech by far negative ids), lora_down (X), beats_gate (qkv),
                qformer_window_xattn (q, out by stride; kv by rows_per_audio = 2^25 + 8 rows of 128)
  decode tail   argmax_eos, argmax_fsm, cross_entropy, sample_eos (logits and work), beam_step at K = 2 (rows_per_batch * ldl):
                logits rows far (stride), B = 2, V = 257 (512 for the automaton's vocabulary); beam_step with
                num_beams * V >= 2^31 - 1 is refused and writes nothing
  GEMMs         gemm: A / C (bf16, f32) / residual (f32, bf16) far each alone and all together, in-place residual, W by ldw; tiles
                1, 2, 3 forced and auto at K = 64 and 256, the row-major (4) and packed (6) skinny kernels, the m128 decode tile
                (5), the fp8-weight skinny kernel, split_k 1 and > 1 (slab reduce), plain / bias + GELU + residual / SwiGLU;
                gemm_rmsnorm: C, residual, xn far, split_k 1 and 4 (splitk_reduce_rmsnorm) and the skinny route; batched form,
                batch = 2 x 256 rows with stride_a / stride_c / stride_r = 2^32 + 64 on tiles 1, 2, 3 (the INTERIOR epilogues: with
                M = 2 only the bounds-checked edge paths run); gemm with the fused RoPE + append epilogue (icl_gemm_rope_kv_bf16):
                A and C rows far (stride), cache rows far (index)
  decode attn   attn_decode and attn_decode_bf16_epl16 (D = 64 and 128, few- and many-sequence instantiations), attn_decode_gqa
                (group 4), attn_decode_fp8: K / V caches in grid-walk form (1030 sequences of 2^22 elements, 260 of 2^24), last
                three lengths 1, 65, 320; attn_decode_rope and attn_decode_rope_fp8: qkv and out rows far (stride), cache rows
                far (index through seq_ids)
  prefill attn  attn_fwd on packed rows with far ldq / ldk / ldv / ldo (stride, lens [1, 1]): D = 64 non-causal (il64), D = 128
                causal, the suffix-query form; attn_fwd on the cache layout in grid-walk form: D = 128 causal, D = 64 non-causal,
                and two query heads on one K/V head (n_kv_heads)
  attn_segmass  Kc in grid-walk form; seg rows by row stride, probs by ld_probs, Q by far q_rows
  kv_copy_spans bf16 and fp8 (bytes and scales): far sequence ids on both sides; a far layer (5-D views whose layer stride is
                2^32 + 64); n_layers = 65536 is refused and writes nothing
  front end     logmel_whisper and fbank_kaldi with two clips at wav_ld = 2^32 + 64

Substituted, and why (the binding is not widened for a test):
  * stride form has M = 2 everywhere (a third row at 2 (2^32 + 64) elements is outside a 16.25 GiB arena for every type but
    uint8); where the index array is tied to those rows there is one near and one far id, the *_many_ids cases have several.
  * W by ldw: two rows (the entry point takes any N; a uniform row stride with more rows puts some at [2^31, 2^32), below the
    pointer under an int32 narrowing).
  * fp8 scale planes are NOT far, in the append, decode and copy cases alike: a plane is indexed by the same cache row r as the
    byte plane, r D bytes there and 4 r here; r >= 2^32 (f32 elements) would put the byte plane at >= 2^38 bytes.  The planes
    sit in the arena at their own r and are compared like every operand.
  * xt_ld of the log-mel output cannot be far: the entry point bounds it to [n_mel, 128]; the refusal is asserted instead.
  * embed_gather_interleave's output has no leading dimension (out + r H), attn_segmass's mass is contiguous by contract: near.
  * lora_down's A and beats_gate's gate stay near (A: r_total <= 64 rows of its own small matrix; gate: M * H contiguous).
  * the fused decode step has two sequences (far qkv rows and far seq_ids need the stride and index forms; the grid-walk form
    needs a thousand qkv rows, which do not fit at a far row stride); packed prefill rows likewise have lens [1, 1].
Not covered: beats_patchify / beats_posconv_pack, whose indices are bounded by clip counts no workload reaches; the load-time
packers (pack_decode_weights, pack_fp8_weights) and spec_to_xt, which the issue does not list.
ref_q (the fp8 contract's rounding) is imported from tests/fp8_ref.py, where it lives.

Wall time of the module on MI355X: 7 s (85 tests; 5 s between the arena's allocation and its release).  Nothing reads or fills
more than its windows; the slowest cases are the grid-walk ones, whose twins are 84 MB.
"""
import time
import zlib

import pytest
import torch

import far_layout as fl
from decoder_support import GOLDEN, fsm_step_reference
from fp8_ref import ref_q
from gpu_support import DEV, B, dev, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8, "i32": torch.int32}
F32, BF16, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8
EPS = 1e-5


@pytest.fixture(scope="module")
def arena():
    free = torch.cuda.mem_get_info()[0]
    need = fl.ARENA_BYTES + (4 << 30)
    if free < need:
        pytest.skip(f"free device memory {free} B is below the arena + 4 GiB = {need} B")
    t0 = time.time()
    a = torch.empty(fl.ARENA_BYTES, dtype=U8, device=DEV)
    yield a
    del a
    torch.cuda.empty_cache()
    print(f"\nfar-offset module wall time: {time.time() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------------
# one launch's memory: the far views into the arena, or the compact twin in buffers of its own
# ------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


ROW_DATA = {}          # group -> f(case, op, i) for the groups whose inputs are not plain random rows


def _row_data(case, o, i):
    """The values of input row i of operand o: the same in the far launch and in the twin."""
    if case.group in ROW_DATA:
        return ROW_DATA[case.group](case, o, i)
    g = _gen(case.name, o.name, i)
    if o.dtype == "u8":
        return torch.randint(0, 0x78, (o.n,), generator=g).to(U8)            # finite e4m3fn codes
    scale = {"w": 0.1}.get(o.name, 1.0)
    return (torch.randn(o.n, generator=g) * scale).to(DT[o.dtype])


def _out_fill(t):
    t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0xFF if t.dtype == U8 else -7)


def _bits(t):
    return t.contiguous().view(-1).view(U8)


class Mem:
    def __init__(self, case, far, arena):
        self.case, self.far, self.dev = case, far, DEV
        self.buf, self.base, self.inputs, self._before = {}, {}, {}, {}
        for o in case.ops:
            offs = self.offs(o.name)
            wins = o.windows(offs)
            if far:
                buf, base = arena, o.base
            else:
                base = fl.MARGIN
                buf = torch.empty(base + wins[-1][1], dtype=U8, device=DEV)
            assert base + wins[0][0] >= 0 and base + wins[-1][1] <= buf.numel()
            self.buf[o.name], self.base[o.name] = buf, base
            for lo, hi in wins:
                buf[base + lo:base + hi].fill_(fl.SENTINEL)
            for i, off in enumerate(offs):
                row = self.row(o.name, off)
                if o.role == "out":
                    _out_fill(row)
                else:
                    self.inputs[(o.name, i)] = _row_data(case, o, i)
                    row.copy_(self.inputs[(o.name, i)])
            self._before[o.name] = [buf[base + lo:base + hi].cpu() for lo, hi in wins]

    def offs(self, name):
        o = self.case.op(name)
        return o.offs if self.far else o.twin

    def meta(self, name, key):
        m = self.case.op(name).meta
        return m[key] if self.far else m[key + "_twin"]

    def row(self, name, off):
        o = self.case.op(name)
        start = self.base[name] + off * o.esize
        return self.buf[name][start:start + o.n * o.esize].view(DT[o.dtype])

    def ptr(self, name):
        """A 1-D tensor of the operand's type that starts at its pointer and reaches to the end of the buffer."""
        o = self.case.op(name)
        buf, base = self.buf[name], self.base[name]
        return buf[base:base + (buf.numel() - base) // o.esize * o.esize].view(DT[o.dtype])

    def rows2d(self, name, rows=None):
        """[rows, n] with the operand's leading dimension (LD_FAR in the far launch of a stride-form operand)."""
        o = self.case.op(name)
        rows = len(o.offs) if rows is None else rows
        return self.ptr(name).as_strided((rows, o.n), (self.meta(name, "ld"), 1))

    def input2d(self, name):
        o = self.case.op(name)
        return torch.stack([self.inputs[(name, i)] for i in range(len(o.offs))])

    def finish(self):
        """(output rows read at their true places, violations of assertion 3)."""
        if self.dev == "cuda":
            torch.cuda.synchronize()
        outs, bad = {}, []
        for o in self.case.ops:
            offs, base, buf = self.offs(o.name), self.base[o.name], self.buf[o.name]
            if o.role != "in":
                for i, off in enumerate(offs):
                    outs[(o.name, i)] = self.row(o.name, off).cpu()
            exp = o.expected(offs)
            for (lo, hi), before in zip(o.windows(offs), self._before[o.name]):
                after = buf[base + lo:base + hi].cpu()
                keep = torch.ones(hi - lo, dtype=torch.bool)
                for a, b in exp:
                    keep[max(a - lo, 0):max(min(b - lo, hi - lo), 0)] = False
                diff = (after != before) & keep
                if bool(diff.any()):
                    at = lo + int(diff.nonzero()[0])
                    bad.append(f"{o.name}: {int(diff.sum())} bytes outside the expected outputs changed, first at byte {at} "
                               f"(element {at // o.esize}) from its pointer")
        return outs, bad


def run_case(B, arena, case, launch, check):
    """The twin launch and the three assertions."""
    mf = Mem(case, True, arena)
    aux_f = launch(B, case, mf) or {}
    out_f, bad_f = mf.finish()
    mt = Mem(case, False, None)
    aux_t = launch(B, case, mt) or {}
    out_t, bad_t = mt.finish()
    aux_f = {k: v.cpu() for k, v in aux_f.items()}
    aux_t = {k: v.cpu() for k, v in aux_t.items()}
    fails = []
    for k in sorted(out_t, key=str):                                         # 1: bit-identical to the twin
        if not torch.equal(_bits(out_f[k]), _bits(out_t[k])):
            d = _bits(out_f[k]) != _bits(out_t[k])
            fails.append(f"(1) {k[0]} row {k[1]}: {int(d.sum())} bytes differ from the twin, first at element "
                         f"{int(d.nonzero()[0]) // case.op(k[0]).esize}: far {out_f[k].view(-1)[int(d.nonzero()[0]) // case.op(k[0]).esize]}")
    for k in sorted(aux_t):
        if not torch.equal(_bits(aux_f[k]), _bits(aux_t[k])):
            fails.append(f"(1) {k}: far {aux_f[k].flatten()[:8].tolist()} != twin {aux_t[k].flatten()[:8].tolist()}")
    fails += [f"(3) far launch, {b}" for b in bad_f] + [f"(3) twin launch, {b}" for b in bad_t]
    assert not fails, f"{case.name}: " + "; ".join(fails[:6])
    check(B, case, mt, out_t, aux_t)                                          # 2: the twin against float64


def _stack(outs, name, n):
    return torch.stack([outs[(name, i)] for i in range(n)])


# ------------------------------------------------------------------------------------------------------------------
# norms
# ------------------------------------------------------------------------------------------------------------------
def _norm_params(N):
    g = _gen("norm", N)
    return 1 + 0.5 * torch.randn(N, generator=g), torch.randn(N, generator=g)


def _launch_norm(B, c, m):
    g, b = dev(*_norm_params(c.p["N"]))
    has = {o.name for o in c.ops}
    x, y = m.rows2d("x"), m.rows2d("y")
    if c.p["rms"]:
        B.rmsnorm(x, g, y, EPS)
    else:
        B.layernorm(x, g, b, y, EPS, res=m.rows2d("res") if "res" in has else None, alpha=0.5,
                    out2=m.rows2d("y2") if "y2" in has else None)


def _check_norm(B, c, m, outs, aux):
    import fp64_bounds as fb
    g, b = _norm_params(c.p["N"])
    has = {o.name for o in c.ops}
    res = m.input2d("res") if "res" in has else None
    y = _stack(outs, "y", 2)
    ref, e = fb.norm_ref_bound(m.input2d("x"), g, b, EPS, rms=c.p["rms"], res=res, alpha=0.5)
    if y.dtype == BF16:
        e = fb.bf16_out_bound(e, ref, y)
    fb.assert_within(y, ref, e, c.name)
    if "y2" in has:
        assert torch.equal(_bits(_stack(outs, "y2", 2)), _bits(y.to(BF16))), f"{c.name}: out2 != bf16(out)"


@pytest.mark.parametrize("case", fl.group("norm"), ids=lambda c: c.name)
def test_norms(B, arena, case):
    run_case(B, arena, case, _launch_norm, _check_norm)


# ------------------------------------------------------------------------------------------------------------------
# RoPE + KV append
# ------------------------------------------------------------------------------------------------------------------
def _rope_args(c):
    import qknorm_ref as qr
    H, Hkv, D = c.p["H"], c.p["Hkv"], c.p["D"]
    cos, sin = qr.rope_tables(D, fl.ROPE_MAXLEN)
    g = _gen("qk gamma")
    gq, gk = 1.0 + 0.3 * torch.randn(D, generator=g), 1.0 + 0.3 * torch.randn(D, generator=g)
    return H, Hkv, D, H * D, (H + Hkv) * D, cos, sin, gq, gk


def _launch_rope(B, c, m, name=None, pos=None):
    import qknorm_ref as qr
    H, Hkv, D, k_off, v_off, cos, sin, gq, gk = _rope_args(c)
    cos, sin, gq, gk = dev(cos, sin, gq, gk)
    p = torch.tensor(c.p["pos"] if pos is None else pos, dtype=I32, device=DEV)
    sid = torch.tensor(m.meta("kc", "ids"), dtype=I32, device=DEV)
    qkv, kc, vc = m.rows2d("qkv"), m.ptr("kc"), m.ptr("vc")
    name = name or c.p["entry"]
    if name == "rope_kv":
        B.rope_kv(qkv, k_off, v_off, cos, sin, p, sid, kc, vc, H, D, fl.ROPE_MAXLEN)
    elif name == "rope_kv_gqa":
        B.rope_kv_gqa(qkv, k_off, v_off, cos, sin, p, sid, kc, vc, H, Hkv, D, fl.ROPE_MAXLEN)
    elif name == "qknorm_rope_kv":
        B.qknorm_rope_kv(qkv, k_off, v_off, gq, gk, qr.EPS, cos, sin, p, sid, kc, vc, H, Hkv, D, fl.ROPE_MAXLEN)
    elif name == "rope_kv_fp8":
        B.rope_kv_fp8(qkv, k_off, v_off, cos, sin, p, sid, kc, vc, m.ptr("ks"), m.ptr("vs"), H, D, fl.ROPE_MAXLEN)
    else:
        B.kv_append_fp8(qkv, k_off, v_off, p, sid, kc, vc, m.ptr("ks"), m.ptr("vs"), H, D, fl.ROPE_MAXLEN)


def _check_rope(B, c, m, outs, aux):
    import fp64_bounds as fb
    import qknorm_ref as qr
    H, Hkv, D, k_off, v_off, cos, sin, gq, gk = _rope_args(c)
    M = c.p["M"]
    orig = m.input2d("qkv")
    entry = c.p["entry"]
    got = _stack(outs, "qkv", M) if entry != "kv_append_fp8" else orig
    pos = torch.tensor(c.p["pos"])
    cs, sn = cos[pos][:, None], sin[pos][:, None]
    blocks = lambda t: (t[:, :k_off].view(M, H, D), t[:, k_off:v_off].view(M, Hkv, D), t[:, v_off:].view(M, Hkv, D))
    q0, k0, v0 = blocks(orig)
    q1, k1, v1 = blocks(got)
    cache = lambda nm: torch.stack([outs[(nm, i)] for i in range(M * Hkv)]).view(M, Hkv, -1)
    assert torch.equal(_bits(v1), _bits(v0)), f"{c.name}: the v block of qkv changed"
    if entry in ("rope_kv", "rope_kv_gqa"):
        for what, x, o in (("q", q0, q1), ("k", k0, k1)):
            ref, e = fb.rope_ref_bound(x, cs, sn)
            lo, hi = fb.bf16_interval(ref, e)
            assert bool(fb.in_interval(o, lo, hi).all()), f"{c.name}: {what} outside the RoPE interval"
        assert torch.equal(_bits(cache("kc")), _bits(k1)) and torch.equal(_bits(cache("vc")), _bits(v0)), f"{c.name}: cache rows"
    elif entry == "qknorm_rope_kv":
        # the project's two stages (tests/test_gpu_qknorm.py): the norm alone at position 0 against float64, then bit equality
        # (+0 = -0) with rope_kv_gqa on a buffer that holds the normalised rows
        m0 = Mem(c, False, None)
        _launch_rope(B, c, m0, pos=(0, 0))
        n, _ = m0.finish()
        nq, nk, _ = blocks(_stack(n, "qkv", M))
        bad_q, _ = qr.norm_check(nq, q0, gq, qr.EPS)
        bad_k, _ = qr.norm_check(nk, k0, gk, qr.EPS)
        assert int(bad_q.sum()) == 0 and int(bad_k.sum()) == 0, f"{c.name}: normalised rows outside the float64 interval"
        m1 = Mem(c, False, None)
        for i in range(M):
            m1.row("qkv", m1.offs("qkv")[i]).copy_(torch.cat([nq[i].flatten(), nk[i].flatten(), v0[i].flatten()]))
        _launch_rope(B, c, m1, name="rope_kv_gqa")
        r, _ = m1.finish()
        assert qr.same_values(_stack(r, "qkv", M), got), f"{c.name}: differs from rope_kv_gqa on the normalised rows"
        assert qr.same_values(cache("kc"), k1) and torch.equal(_bits(cache("vc")), _bits(v0)), f"{c.name}: cache rows"
    else:
        # fp8 forms, by their anchor: q rotated as rope_kv rotates it (k left alone), the planes hold ref_q of the rotated k / of v
        k_rot = k0
        if entry == "rope_kv_fp8":
            ca = fl.BY_NAME["rope_kv"]                       # the same shapes with bf16 caches
            assert (ca.p["H"], ca.p["Hkv"], ca.p["D"], ca.p["M"]) == (H, Hkv, D, M)
            ma = Mem(ca, False, None)
            for i in range(M):
                ma.row("qkv", ma.offs("qkv")[i]).copy_(orig[i])
            _launch_rope(B, ca, ma)
            ra, _ = ma.finish()
            qa, k_rot, _ = blocks(_stack(ra, "qkv", M))
            assert torch.equal(_bits(q1), _bits(qa)), f"{c.name}: q is not what rope_kv makes of it"
            assert torch.equal(_bits(k1), _bits(k0)), f"{c.name}: the k block of qkv changed"
        for nm, sc, rows in (("kc", "ks", k_rot), ("vc", "vs", v0)):
            rb, rs, _ = ref_q(rows)
            assert torch.equal(cache(nm), rb), f"{c.name}: {nm} bytes differ from the contract's rounding"
            assert torch.equal(cache(sc).view(M, Hkv), rs), f"{c.name}: {sc} scales differ from the contract's"


@pytest.mark.parametrize("case", fl.group("rope"), ids=lambda c: c.name)
def test_rope_kv_append(B, arena, case):
    run_case(B, arena, case, _launch_rope, _check_rope)


# ------------------------------------------------------------------------------------------------------------------
# glue
# ------------------------------------------------------------------------------------------------------------------
GATE_SEEDS = (52, 53, 54)


def _gate_params():
    w = torch.randn(8, 64, generator=torch.Generator().manual_seed(GATE_SEEDS[0])) * 0.2
    b = torch.randn(8, generator=torch.Generator().manual_seed(GATE_SEEDS[1]))
    a = torch.rand(12, generator=torch.Generator().manual_seed(GATE_SEEDS[2])) + 0.5
    return w, b, a


def _launch_glue(B, c, m):
    if c.name.startswith("gather_rows"):
        idx = torch.tensor(m.meta("src", "ids"), dtype=I32, device=DEV)
        src = m.ptr("src").as_strided((max(m.meta("src", "ids")) + 1, c.p["N"]), (c.p["N"], 1))
        B.gather_rows(src, idx, m.rows2d("out"))
    elif c.name.startswith("axpby_cast"):
        B.axpby_cast(m.rows2d("x"), m.rows2d("out"), alpha=0.3, add=m.rows2d("add"))
    elif c.name == "embed_gather_interleave":
        H = c.p["H"]
        ids = [m.meta(nm, "ids")[i] if nm == "table" else -m.meta(nm, "ids")[i] - 1 for nm, i in c.p["order"]]
        view = lambda nm: m.ptr(nm).as_strided((max(m.meta(nm, "ids")) + 1, H), (H, 1))
        B.embed_gather_interleave(torch.tensor(ids, dtype=I32, device=DEV), view("table"), view("speech"), m.rows2d("out"))
    elif c.name == "lora_down":
        B.lora_down(m.rows2d("x"), c.p["K0"], m.rows2d("a"), c.p["r"], 2.0)
    else:
        w, b, a = dev(*_gate_params())
        B.beats_gate(m.rows2d("qkv"), w, b, a, m.ptr("gate")[:2 * c.p["H"]], c.p["H"])


def _interval(fb, out, ref, e, what):
    lo, hi = fb.bf16_interval(ref, e)
    assert bool(fb.in_interval(out, lo, hi).all()), f"{what}: outside [bf16(ref - e), bf16(ref + e)]"


def _check_glue(B, c, m, outs, aux):
    import fp64_bounds as fb
    if c.name.startswith("gather_rows"):
        assert torch.equal(_bits(_stack(outs, "out", 2)), _bits(m.input2d("src"))), f"{c.name}: rows are not copies"
    elif c.name.startswith("axpby_cast"):
        out = _stack(outs, "out", 2)
        ref, e = fb.axpby_ref_bound(m.input2d("x"), 0.3, m.input2d("add"))
        _interval(fb, out, ref, e, c.name) if out.dtype == BF16 else fb.assert_within(out, ref, e, c.name)
    elif c.name == "embed_gather_interleave":
        want = torch.stack([m.inputs[(nm, i)].float() for nm, i in c.p["order"]])
        assert torch.equal(_bits(_stack(outs, "out", 8)), _bits(want)), f"{c.name}: rows are not the table's / the speech rows"
    elif c.name == "lora_down":
        K0, r = c.p["K0"], c.p["r"]
        x, a, got = m.input2d("x"), m.input2d("a"), _stack(outs, "x", 2)
        ref, e = fb.lora_ref_bound(x[:, :K0], a, 2.0)
        _interval(fb, got[:, K0:K0 + r], ref, e, c.name)
        assert torch.equal(_bits(got[:, :K0]), _bits(x[:, :K0])), f"{c.name}: the K0 input columns changed"
    else:
        H = c.p["H"]
        ref, e = fb.gate_ref_bound(m.input2d("qkv").view(2, H, 64), *_gate_params())
        fb.assert_within(_stack(outs, "gate", 2), ref, e, c.name)


@pytest.mark.parametrize("case", fl.group("glue"), ids=lambda c: c.name)
def test_glue(B, arena, case):
    run_case(B, arena, case, _launch_glue, _check_glue)


# ------------------------------------------------------------------------------------------------------------------
# decode tail and loss
# ------------------------------------------------------------------------------------------------------------------
SAMPLE_CAP, SAMPLE_SENT = 1024, -12345.5
BEAM = dict(B=1, K=2, T=4, step=1, eos=3, lp=1.0, pen=1.0, rows=2)
_BEAM_STATE = ("run_score", "run_seq", "fin_score", "fin_seq", "fin_len", "fin_flag", "unsat")


def _sample_case(c, rows):
    """The launch as a case dict of tests/decode_tail_cases.py (what fb.check_sampler_row reads)."""
    import numpy as np
    import decode_tail_cases as dc
    tk = np.full((2, 8), 7, np.int32)
    tk[:, :2] = [[5, 9], [5, 300]]                        # two previous tokens per row; 300 >= V is ignored by the penalty
    return dc._case("far", rows, step=2, width=8, temp=0.8, top_k=50, top_p=0.9, pen=1.3, u=np.array([0.3, 0.7], np.float32), tokens=tk)


def _beam_state0(B, V):
    """The state one step-0 launch of the kernel leaves on seeded near logits (its own history, as the project's search test)."""
    st = B.BeamState(lambda name, shape, dt: torch.empty(shape, dtype=dt, device=DEV), BEAM["B"], BEAM["K"], BEAM["T"], pad_id=0)
    lg0 = (torch.randn(1, V, generator=_gen("beam step 0")) * 2).to(DEV)
    B.beam_step(lg0, st, 0, BEAM["eos"], BEAM["lp"], repetition_penalty=BEAM["pen"])
    return st


FSM_STEPS_LEFT, FSM_EOS, FSM_PAD = 10, 2, 400
_FSM = {}


def _automaton():
    """The label automaton of tests/test_gpu_constrained.py (every typed task of the 401-token test tokenizer)."""
    if not _FSM:
        import os
        from icl_speech_text_llm_amd.data.task_configs import DatasetType
        from icl_speech_text_llm_amd.runtime.constraints import build_label_automaton
        from icl_speech_text_llm_amd.utils.tokenization import load_llama_tokenizer
        a = build_label_automaton(load_llama_tokenizer(os.path.join(GOLDEN, "llama_spm"), 401), list(DatasetType))
        start = next(s for s in a.starts.values() if s >= 0 and a.min_tokens(s) <= FSM_STEPS_LEFT)
        _FSM.update(a=a, states=[start, -1])                    # row 0 constrained from a start state, row 1 free
    return _FSM["a"], _FSM["states"]


def _launch_tail(B, c, m):
    logits = m.rows2d("logits")
    if c.name == "argmax_fsm":
        a, states = _automaton()
        st = torch.tensor(states, dtype=I32, device=DEV)
        fin = torch.zeros(2, dtype=I32, device=DEV)
        toks = torch.full((2, 4), -9, dtype=I32, device=DEV)
        lps = torch.full((2, 4), 7.0, dtype=F32, device=DEV)
        nxt = torch.full((2,), -9, dtype=I32, device=DEV)
        B.argmax_fsm(logits, a.upload(DEV), st, FSM_STEPS_LEFT, FSM_EOS, FSM_PAD, fin, toks, 1, nxt, out_logprob=lps)
        return dict(state=st, finished=fin, tokens=toks, logprob=lps, next_ids=nxt)
    if c.name == "sample_eos":
        s = _sample_case(c, m.input2d("logits").numpy())
        toks = torch.from_numpy(s["tokens"]).to(DEV)
        fin, nxt = torch.zeros(2, dtype=I32, device=DEV), torch.full((2,), -7, dtype=I32, device=DEV)
        ids = torch.full((2, SAMPLE_CAP), -1, dtype=I32, device=DEV)
        probs = torch.full((2, SAMPLE_CAP), SAMPLE_SENT, dtype=F32, device=DEV)
        cnt = torch.full((2,), -9, dtype=I32, device=DEV)
        B.sample_eos(logits, m.rows2d("work"), torch.from_numpy(s["u"]).to(DEV), s["eos"], s["pad"], fin, toks, s["step"], nxt,
                     temperature=s["temp"], top_k=s["top_k"], top_p=s["top_p"], repetition_penalty=s["pen"], debug=(ids, probs, cnt))
        return dict(tokens=toks, finished=fin, next_id=nxt, ids=ids, probs=probs, count=cnt)
    if c.name == "beam_step_k2":
        st = _beam_state0(B, c.p["V"])
        aux = {"old_" + k: getattr(st, k).clone() for k in _BEAM_STATE}
        st.next_ids.fill_(-5)
        st.parent.fill_(-5)
        B.beam_step(logits, st, BEAM["step"], BEAM["eos"], BEAM["lp"], repetition_penalty=BEAM["pen"])
        aux.update({"new_" + k: getattr(st, k) for k in _BEAM_STATE})
        return dict(aux, next_ids=st.next_ids, parent=st.parent)
    if c.name == "argmax_eos":
        fin = torch.zeros(2, dtype=I32, device=DEV)
        toks = torch.full((2, 4), -5, dtype=I32, device=DEV)
        nxt = torch.full((2,), -5, dtype=I32, device=DEV)
        B.argmax_eos(logits, 300, 0, fin, toks, 1, nxt)
        return dict(finished=fin, tokens=toks, next_ids=nxt)
    labels = torch.tensor([3, c.p["V"] - 1], dtype=I32, device=DEV)
    rows = torch.full((2,), float("nan"), dtype=F32, device=DEV)
    mean = torch.full((1,), float("nan"), dtype=F32, device=DEV)
    B.cross_entropy(logits, labels, rows, mean)
    return dict(row_loss=rows, mean_loss=mean)


def _check_tail(B, c, m, outs, aux):
    import fp64_bounds as fb
    x = m.input2d("logits")
    if c.name == "argmax_fsm":
        a, states = _automaton()
        for b in range(2):                          # the numpy stepper; the log-probability bound of tests/test_gpu_constrained.py
            t, n, lp = fsm_step_reference(x[b].numpy(), states[b], FSM_STEPS_LEFT, a)
            got = (int(aux["tokens"][b, 1]), int(aux["state"][b]), int(aux["next_ids"][b]), int(aux["finished"][b]))
            assert got == (t, n, t, int(t == FSM_EOS)), (b, got, (t, n, lp))
            assert abs(float(aux["logprob"][b, 1]) - lp) <= 1e-5 * max(1.0, abs(lp)), (b, float(aux["logprob"][b, 1]), lp)
        assert bool((aux["tokens"][:, [0, 2, 3]] == -9).all()) and bool((aux["logprob"][:, [0, 2, 3]] == 7.0).all())
        return
    if c.name == "sample_eos":
        s = _sample_case(c, x.numpy())
        for b in range(2):
            out = {k: aux[k][b].numpy() for k in ("tokens", "finished", "next_id", "ids", "probs", "count")}
            fb.check_sampler_row(s, b, dict(out, work=outs[("work", b)].numpy()), f"{c.name}[{b}]")
        return
    if c.name == "beam_step_k2":
        import decode_tail_cases as dc
        params = dict(BEAM, V=c.p["V"])
        old = dc.beam_row_view({k: aux["old_" + k].numpy() for k in _BEAM_STATE}, 0)
        row = dc.beam_row_view({k: aux["new_" + k].numpy() for k in _BEAM_STATE}, 0)
        row.update(next_ids=aux["next_ids"].numpy().reshape(1, 2)[0], parent=aux["parent"].numpy().reshape(1, 2)[0])
        fb.check_beam_row(dc.beam_row_ref(params, x.numpy(), old), row, old, c.name)
        return
    if c.name == "argmax_eos":
        want = x.double().argmax(-1).tolist()
        assert len(set(want)) == 2                              # a launch that reads row 0 twice shows
        assert aux["next_ids"].tolist() == want and aux["tokens"][:, 1].tolist() == want and aux["finished"].tolist() == [0, 0]
        assert aux["tokens"][:, [0, 2, 3]].eq(-5).all()
        return
    ref, e, mref, me = fb.ce_ref_bound(x, torch.tensor([3, c.p["V"] - 1], dtype=I32))
    fb.assert_within(aux["row_loss"], ref, e, c.name)
    assert abs(float(aux["mean_loss"]) - mref) <= me


@pytest.mark.parametrize("case", fl.group("tail"), ids=lambda c: c.name)
def test_decode_tail_and_loss(B, arena, case):
    run_case(B, arena, case, _launch_tail, _check_tail)


def test_beam_step_refuses_a_flat_index_beyond_int32(B, arena):
    """num_beams * V >= 2^31 - 1 (two beams over rows of 2^30 logits, views into the arena) is refused by the argument check, and
    neither the state nor the arena is written: a refusal is a pass, a silent wrap is not."""
    c = fl.BY_NAME["beam_step_k2"]
    m = Mem(c, True, arena)
    st = _beam_state0(B, c.p["V"])
    before = {k: getattr(st, k).clone() for k in _BEAM_STATE + ("next_ids", "parent")}
    V = 1 << 30
    wide = m.ptr("logits").as_strided((2, V), (V, 1))
    with pytest.raises(B.IclError, match="overflows the flat index"):
        B.beam_step(wide, st, 1, BEAM["eos"], BEAM["lp"])
    _, bad = m.finish()
    assert not bad and all(torch.equal(_bits(getattr(st, k)), _bits(v)) for k, v in before.items()), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# GEMMs
# ------------------------------------------------------------------------------------------------------------------
def _gemm_weights(c):
    """(w bf16 [N, K], bias f32 [N]); the stride-form W case takes its two rows from the arena instead."""
    g = _gen("gemm w", c.p["N"], c.p["K"])
    return (torch.randn(c.p["N"], c.p["K"], generator=g) * 0.1).to(BF16), torch.randn(c.p["N"], generator=g)


def _launch_gemm(B, c, m):
    N, K, tile, split_k, epi = (c.p[k] for k in ("N", "K", "tile", "split_k", "epi"))
    has = {o.name for o in c.ops}
    w, bias = dev(*_gemm_weights(c))
    kw = dict(split_k=split_k, N=N, K=K)
    if "w" in has:
        w = m.rows2d("w")
    if tile == "fp8w":
        w, kw["w_scale"], _ = B.pack_fp8_weights(w)
    else:
        kw["tile"] = tile
        if tile in (5, 6):
            w = B.pack_decode_weights(w)
    if split_k > 1:
        kw["workspace"] = torch.full((split_k * 2 * N,), float("nan"), dtype=F32, device=DEV)
    out = m.rows2d("c")
    if epi == "bias_gelu_res":
        kw.update(bias=bias, gelu=True, residual=m.rows2d("r"))
    elif epi == "plain_res":
        kw.update(residual=out if c.p["inplace"] else m.rows2d("r"))
    elif epi == "swiglu":
        kw.update(swiglu=True)
    B.gemm(m.rows2d("a"), w, out, **kw)


def _gemm_ref(B, c, m):
    """(dot, mag) in float64 with the weights the kernel used (the fp8 form: W' = q * 2^e, exact in bf16)."""
    import fp64_bounds as fb
    w, bias = _gemm_weights(c)
    if any(o.name == "w" for o in c.ops):
        w = m.input2d("w")
    if c.p.get("tile") == "fp8w":
        w = B.pack_fp8_weights(w.to(DEV))[2].cpu()
    return fb.dot64(m.input2d("a"), w), bias


def _check_gemm(B, c, m, outs, aux):
    import fp64_bounds as fb
    K, epi = c.p["K"], c.p["epi"]
    (dot, mag), bias = _gemm_ref(B, c, m)
    got = _stack(outs, "c", 2)
    if epi == "swiglu":
        ref, e = fb.swiglu_ref_bound(dot, mag, K)
    elif epi == "bias_gelu_res":
        ref, e = fb.gemm_ref_bound(dot, mag, K, bias=bias, residual=m.input2d("r"), gelu=True)
    elif epi == "plain_res":
        ref, e = fb.gemm_ref_bound(dot, mag, K, residual=m.input2d("c" if c.p["inplace"] else "r"))
    else:
        ref, e = fb.gemm_ref_bound(dot, mag, K)
    if got.dtype == BF16:
        e = fb.bf16_out_bound(e, ref, got)
    fb.assert_within(got, ref, e, c.name)


@pytest.mark.parametrize("case", fl.group("gemm"), ids=lambda c: c.name)
def test_gemm(B, arena, case):
    run_case(B, arena, case, _launch_gemm, _check_gemm)


def _launch_gemm_rmsnorm(B, c, m):
    N, K, tile, split_k = (c.p[k] for k in ("N", "K", "tile", "split_k"))
    w, _ = dev(*_gemm_weights(c))
    gamma = _norm_params(N)[0].to(DEV)
    ws = torch.full((split_k * 2 * N,), float("nan"), dtype=F32, device=DEV) if split_k > 1 else None
    B.gemm_rmsnorm(m.rows2d("a"), w, m.rows2d("c"), gamma, EPS, m.rows2d("xn"), residual=m.rows2d("r"), split_k=split_k,
                   workspace=ws, tile=tile, N=N, K=K)


def _check_gemm_rmsnorm(B, c, m, outs, aux):
    import fp64_bounds as fb
    (dot, mag), _ = _gemm_ref(B, c, m)
    got, xn = _stack(outs, "c", 2), _stack(outs, "xn", 2)
    ref, e = fb.gemm_ref_bound(dot, mag, c.p["K"], residual=m.input2d("r"))
    fb.assert_within(got, ref, e, c.name + " C")
    gamma = _norm_params(c.p["N"])[0]
    nref, ne = fb.norm_ref_bound(got, gamma, None, EPS, rms=True)          # the row the kernel normalised, taken as data
    fb.assert_within(xn, nref, fb.bf16_out_bound(ne, nref, xn), c.name + " xn")


@pytest.mark.parametrize("case", fl.group("gemm_rmsnorm"), ids=lambda c: c.name)
def test_gemm_rmsnorm(B, arena, case):
    run_case(B, arena, case, _launch_gemm_rmsnorm, _check_gemm_rmsnorm)


def _launch_gemm_batched(B, c, m):
    w, bias = dev(*_gemm_weights(c))

    has = {o.name for o in c.ops}
    M, epi = c.p["M"], c.p["epi"]

    def view(nm):                                 # batch 0: [M, ld] contiguous; the batch stride goes by argument
        ld = m.meta(nm, "ld")
        return m.ptr(nm).as_strided((M, ld), (ld, 1))
    kw = dict(bias=bias, batch=2, tile=c.p["tile"], stride_a=m.meta("a", "stride"), stride_c=m.meta("c", "stride"))
    if "r" in has:
        kw.update(residual=view("r"), stride_r=m.meta("r", "stride"))
    B.gemm(view("a"), w, view("c"), gelu=epi == "bias_gelu_res", swiglu=epi == "swiglu", **kw)


def _check_gemm_batched(B, c, m, outs, aux):
    import fp64_bounds as fb
    M, K, epi = c.p["M"], c.p["K"], c.p["epi"]
    w, bias = _gemm_weights(c)
    dot, mag = fb.dot64(m.input2d("a").view(2, M, K), w)
    got = _stack(outs, "c", 2).view(2, M, -1)
    res = m.input2d("r").view(2, M, -1) if any(o.name == "r" for o in c.ops) else None
    if epi == "swiglu":
        ref, e = fb.swiglu_ref_bound(dot, mag, K, bias=bias)
    else:
        ref, e = fb.gemm_ref_bound(dot, mag, K, bias=bias, residual=res, gelu=epi == "bias_gelu_res")
    if got.dtype == BF16:
        e = fb.bf16_out_bound(e, ref, got)
    fb.assert_within(got.reshape(2 * M, -1), ref.reshape(2 * M, -1), e.reshape(2 * M, -1), c.name)


@pytest.mark.parametrize("case", fl.group("gemm_batched"), ids=lambda c: c.name)
def test_gemm_batched(B, arena, case):
    run_case(B, arena, case, _launch_gemm_batched, _check_gemm_batched)


# ------------------------------------------------------------------------------------------------------------------
# decode attention: the caches in grid-walk form
# ------------------------------------------------------------------------------------------------------------------
def _decode_q(c):
    _, nseq = c.p["geom"]
    return torch.randn(nseq, c.p["H"] * c.p["D"], generator=_gen("decode q", c.name)).to(BF16)


def _launch_decode(B, c, m):
    # The launch walks ALL sequences.  The unchecked ones (length 1) read one position of arena memory nobody initialised, maybe
    # what an earlier case left there; their output rows are discarded.  A narrowing that sends a CHECKED sequence onto such a
    # stripe is still seen, because the layout makes every place a checked row can narrow to a sentinel-filled window of its own.
    D, H = c.p["D"], c.p["H"]
    geom = c.p["geom"]
    lens = torch.ones(geom[1], dtype=I32)
    for s, n in fl.grid_checked(geom).items():
        lens[s] = n
    q = _decode_q(c).to(DEV)
    out = torch.full_like(q, float("nan"))
    fn = B.attn_decode_bf16_epl16 if "epl16" in c.name else B.attn_decode
    fn(q, m.ptr("kc"), m.ptr("vc"), out, lens.to(DEV), H, D, m.meta("kc", "max_len"), D ** -0.5)
    checked = torch.tensor(list(fl.grid_checked(geom)), device=DEV)
    return dict(out=out[checked])


def _check_decode(B, c, m, outs, aux):
    from oracle import attention as oa
    D, H = c.p["D"], c.p["H"]
    chk = fl.grid_checked(c.p["geom"])
    q = _decode_q(c)[list(chk)]
    kc = m.input2d("kc").view(len(chk), H, fl.GRID_ROWS, D)
    vc = m.input2d("vc").view(len(chk), H, fl.GRID_ROWS, D)
    R = oa.decode_ref(q, kc, vc, list(chk.values()), H, D, D ** -0.5)
    oa.assert_bound(aux["out"].view(len(chk), H, D), R, D, oa.R_P["decode"], c.name)


@pytest.mark.parametrize("case", fl.group("decode"), ids=lambda c: c.name)
def test_decode_attention(B, arena, case):
    run_case(B, arena, case, _launch_decode, _check_decode)


def _grid_lens(c):
    lens = torch.ones(c.p["geom"][1], dtype=I32)
    for s, n in fl.grid_checked(c.p["geom"]).items():
        lens[s] = n
    return lens


def _launch_decode_gqa(B, c, m):
    D, H, Hkv = c.p["D"], c.p["H"], c.p["Hkv"]
    q = _decode_q(c).to(DEV)
    out = torch.full_like(q, float("nan"))
    B.attn_decode_gqa(q, m.ptr("kc"), m.ptr("vc"), out, _grid_lens(c).to(DEV), H, Hkv, D, m.meta("kc", "max_len"), D ** -0.5)
    return dict(out=out[torch.tensor(list(fl.grid_checked(c.p["geom"])), device=DEV)])


def _check_decode_gqa(B, c, m, outs, aux):
    from oracle import attention as oa
    D, H, Hkv = c.p["D"], c.p["H"], c.p["Hkv"]
    chk = fl.grid_checked(c.p["geom"])
    q = _decode_q(c)[list(chk)]
    kc = m.input2d("kc").view(len(chk), Hkv, fl.GRID_ROWS, D).repeat_interleave(H // Hkv, dim=1)     # query head h reads K/V head h / group
    vc = m.input2d("vc").view(len(chk), Hkv, fl.GRID_ROWS, D).repeat_interleave(H // Hkv, dim=1)
    R = oa.decode_ref(q, kc, vc, list(chk.values()), H, D, D ** -0.5)
    oa.assert_bound(aux["out"].view(len(chk), H, D), R, D, oa.R_P["decode"], c.name)


@pytest.mark.parametrize("case", fl.group("decode_gqa"), ids=lambda c: c.name)
def test_decode_attention_gqa(B, arena, case):
    run_case(B, arena, case, _launch_decode_gqa, _check_decode_gqa)


def _fp8_rows(c, which, i):
    """(bytes, scales, x') of the GRID_ROWS cache rows of checked sequence i of the K (which = "k") or V plane: the contract's
    rounding (ref_q of tests/fp8_ref.py) of seeded bf16 rows of very different magnitudes."""
    g = _gen(c.name, which, i)
    mag = torch.exp2(torch.randint(-6, 3, (fl.GRID_ROWS, 1), generator=g).float())
    return ref_q((torch.randn(fl.GRID_ROWS, c.p["D"], generator=g) * mag).to(BF16))


def _fp8_row_data(c, o, i):
    q, s, _ = _fp8_rows(c, o.name[0], i)
    return q.flatten() if o.dtype == "u8" else s


def _launch_decode_fp8(B, c, m):
    D, H = c.p["D"], c.p["H"]
    q = _decode_q(c).to(DEV)
    out = torch.full_like(q, float("nan"))
    B.attn_decode_fp8(q, m.ptr("kc"), m.ptr("vc"), m.ptr("ks"), m.ptr("vs"), out, _grid_lens(c).to(DEV), H, D, m.meta("kc", "max_len"),
                      D ** -0.5)
    return dict(out=out[torch.tensor(list(fl.grid_checked(c.p["geom"])), device=DEV)])


def _check_decode_fp8(B, c, m, outs, aux):
    """The fp8 kernel's anchor: bit for bit the bf16 kernel of the same lane mapping (attn_decode_bf16_epl16) on a bf16 cache of
    x' = byte * scale, with the same number of sequences (the same instantiation)."""
    D, H = c.p["D"], c.p["H"]
    nseq = c.p["geom"][1]
    chk = list(fl.grid_checked(c.p["geom"]))
    kx = torch.zeros(nseq, H, fl.GRID_ROWS, D, dtype=BF16)
    vx = torch.zeros_like(kx)
    for i, s in enumerate(chk):
        kx[s, 0], vx[s, 0] = _fp8_rows(c, "k", i)[2], _fp8_rows(c, "v", i)[2]
        assert torch.equal(m.inputs[("kc", i)], _fp8_rows(c, "k", i)[0].flatten())
    q = _decode_q(c).to(DEV)
    ob = torch.full_like(q, float("nan"))
    B.attn_decode_bf16_epl16(q, kx.to(DEV), vx.to(DEV), ob, _grid_lens(c).to(DEV), H, D, fl.GRID_ROWS, D ** -0.5)
    ob = ob.cpu()[chk]
    assert torch.equal(_bits(aux["out"]), _bits(ob)), f"{c.name}: differs from attn_decode_bf16_epl16 on x'"
    assert bool(torch.isfinite(ob.float()).all())


@pytest.mark.parametrize("case", fl.group("decode_fp8"), ids=lambda c: c.name)
def test_decode_attention_fp8(B, arena, case):
    run_case(B, arena, case, _launch_decode_fp8, _check_decode_fp8)


ROW_DATA["decode_fp8"] = _fp8_row_data


# ------------------------------------------------------------------------------------------------------------------
# the fused decode step: RoPE + append + attention in one launch
# ------------------------------------------------------------------------------------------------------------------
def _fused_args(c):
    import qknorm_ref as qr
    H, D = c.p["H"], c.p["D"]
    cos, sin = qr.rope_tables(D, fl.FUSED_MAXLEN)
    pos = torch.tensor(fl.ROPE_POS, dtype=I32)
    return H, D, H * D, cos, sin, pos, pos + 1


def _launch_fused(B, c, m):
    H, D, hd, cos, sin, pos, lens = _fused_args(c)
    cos, sin, pos, lens = dev(cos, sin, pos, lens)
    sid = torch.tensor(m.meta("kc", "ids"), dtype=I32, device=DEV)
    if c.p["fp8"]:
        B.attn_decode_rope_fp8(m.rows2d("qkv"), hd, 2 * hd, cos, sin, pos, sid, m.ptr("kc"), m.ptr("vc"), m.ptr("ks"), m.ptr("vs"),
                               m.rows2d("out"), lens, H, D, fl.FUSED_MAXLEN, D ** -0.5)
        return
    B.attn_decode_rope(m.rows2d("qkv"), hd, 2 * hd, cos, sin, pos, sid, m.ptr("kc"), m.ptr("vc"), m.rows2d("out"), lens, H, D,
                       fl.FUSED_MAXLEN, D ** -0.5)


def _check_fused(B, c, m, outs, aux):
    """The fused launch's own contract: bit-identical to rope_kv followed by attn_decode (each held to float64 by its own case),
    and the float64 bound of decode attention on the cache as the launch left it."""
    from oracle import attention as oa
    H, D, hd, cos, sin, pos, lens = _fused_args(c)
    T = fl.FUSED_MAXLEN
    if c.p["fp8"]:
        return _check_fused_fp8(B, c, m, outs)
    qkv = m.input2d("qkv").to(DEV)
    kc = m.input2d("kc").view(2, H, T, D).to(DEV)
    vc = m.input2d("vc").view(2, H, T, D).to(DEV)
    sid = torch.arange(2, dtype=I32, device=DEV)
    B.rope_kv(qkv, hd, 2 * hd, cos.to(DEV), sin.to(DEV), pos.to(DEV), sid, kc, vc, H, D, T)
    ref = torch.full((2, hd), float("nan"), dtype=BF16, device=DEV)
    B.attn_decode(qkv[:, :hd].contiguous(), kc, vc, ref, lens.to(DEV), H, D, T, D ** -0.5)
    got = _stack(outs, "out", 2)
    assert torch.equal(_bits(got), _bits(ref.cpu())), f"{c.name}: out differs from rope_kv + attn_decode"
    assert torch.equal(_bits(_stack(outs, "kc", 2 * H)), _bits(kc.cpu())) and torch.equal(_bits(_stack(outs, "vc", 2 * H)), _bits(vc.cpu()))
    R = oa.decode_ref(qkv[:, :hd].cpu(), kc.cpu(), vc.cpu(), lens.tolist(), H, D, D ** -0.5)
    oa.assert_bound(got.view(2, H, D), R, D, oa.R_P["decode"], c.name)


def _fused_fp8_stripe(c, which, i):
    """(bytes, scales, x') of stripe i (sequence i // H, head i % H) of the K or V plane: the contract's rounding of seeded rows."""
    g = _gen(c.name, which, i)
    mag = torch.exp2(torch.randint(-6, 3, (fl.FUSED_MAXLEN, 1), generator=g).float())
    return ref_q((torch.randn(fl.FUSED_MAXLEN, c.p["D"], generator=g) * mag).to(BF16))


def _fused_row_data(c, o, i):
    if not c.p["fp8"] or o.name in ("qkv", "out"):
        return torch.randn(o.n, generator=_gen(c.name, o.name, i)).to(DT[o.dtype])
    q, s, _ = _fused_fp8_stripe(c, o.name[0], i)
    return q.flatten() if o.dtype == "u8" else s


ROW_DATA["decode_rope"] = _fused_row_data


def _check_fused_fp8(B, c, m, outs):
    """The fp8 form's anchor (tests/test_gpu_fp8_kv.py): rope_kv on a bf16 cache holding x', the appended rows replaced by their
    fp8 rounding, then the bf16 kernel of the fp8 kernel's lane mapping: output and appended bytes / scales bit for bit."""
    H, D, hd, cos, sin, pos, lens = _fused_args(c)
    T = fl.FUSED_MAXLEN
    qkv = m.input2d("qkv")
    kx = torch.stack([_fused_fp8_stripe(c, "k", i)[2] for i in range(2 * H)]).view(2, H, T, D).to(DEV)
    vx = torch.stack([_fused_fp8_stripe(c, "v", i)[2] for i in range(2 * H)]).view(2, H, T, D).to(DEV)
    ref = qkv.to(DEV)
    B.rope_kv(ref, hd, 2 * hd, cos.to(DEV), sin.to(DEV), pos.to(DEV), torch.arange(2, dtype=I32, device=DEV), kx, vx, H, D, T)
    p = pos.long()
    for cache in (kx, vx):
        for b in range(2):
            cache[b, :, p[b]] = ref_q(cache[b, :, p[b]].cpu())[2].to(DEV)
    ob = torch.full((2, hd), float("nan"), dtype=BF16, device=DEV)
    B.attn_decode_bf16_epl16(ref[:, :hd].contiguous(), kx, vx, ob, lens.to(DEV), H, D, T, D ** -0.5)
    assert torch.equal(_bits(_stack(outs, "out", 2)), _bits(ob.cpu())), f"{c.name}: out differs from the bf16 kernel on x'"
    assert bool(torch.isfinite(ob.float()).all())
    kb, ksc, _ = ref_q(ref.cpu().view(2, 3, H, D)[:, 1])
    vb, vsc, _ = ref_q(qkv.view(2, 3, H, D)[:, 2])
    for nm, sn, wb, wsc in (("kc", "ks", kb, ksc), ("vc", "vs", vb, vsc)):
        want_b = torch.stack([m.inputs[(nm, i)] for i in range(2 * H)]).view(2, H, T, D).clone()
        want_s = torch.stack([m.inputs[(sn, i)] for i in range(2 * H)]).view(2, H, T).clone()
        for b in range(2):
            want_b[b, :, p[b]], want_s[b, :, p[b]] = wb[b], wsc[b]
        assert torch.equal(_stack(outs, nm, 2 * H).view(2, H, T, D), want_b), f"{c.name}: {nm} is not the old plane + the appended row"
        assert torch.equal(_bits(_stack(outs, sn, 2 * H).view(2, H, T)), _bits(want_s)), f"{c.name}: {sn}"


@pytest.mark.parametrize("case", fl.group("decode_rope"), ids=lambda c: c.name)
def test_fused_decode_step(B, arena, case):
    run_case(B, arena, case, _launch_fused, _check_fused)


# ------------------------------------------------------------------------------------------------------------------
# kv_copy_spans
# ------------------------------------------------------------------------------------------------------------------
def _copy_view(c, m, name, per_pos):
    """The 5-D cache view [layers][seqs][heads][positions][head_dim] (4-D for a scale plane) that spans the operand's sequences."""
    o = c.op(name)
    n_seqs, s_layer = m.meta(name, "n_seqs"), m.meta(name, "s_layer")
    H, T = fl.COPY_H, fl.COPY_T
    shape, stride = (c.p["L"], n_seqs, H, T), (s_layer if c.p["L"] > 1 else n_seqs * H * T * per_pos, H * T * per_pos, T * per_pos, per_pos)
    if per_pos > 1:
        shape, stride = shape + (per_pos,), stride + (1,)
    return m.ptr(o.name).as_strided(shape, stride)


def _launch_copy(B, c, m):
    ids = {side: torch.tensor(m.meta(side, "ids"), dtype=I32, device=DEV) for side in ("src", "dst")}
    t0 = {side: torch.tensor(c.p["t0"][side], dtype=I32, device=DEV) for side in ("src", "dst")}
    kw = dict(src_seq=ids["src"], src_t0=t0["src"], dst_seq=ids["dst"], dst_t0=t0["dst"], n_fixed=fl.COPY_N)
    if c.p["fp8"]:
        kw.update(src_scale=_copy_view(c, m, "src_scale", 1), dst_scale=_copy_view(c, m, "dst_scale", 1))
    B.kv_copy_spans(_copy_view(c, m, "src", fl.COPY_D), _copy_view(c, m, "dst", fl.COPY_D), 2, **kw)


def _check_copy(B, c, m, outs, aux):
    n = c.p["L"] * 2 * fl.COPY_H
    assert torch.equal(_bits(_stack(outs, "dst", n)), _bits(m.input2d("src"))), f"{c.name}: the spans are not copies"
    if c.p["fp8"]:
        assert torch.equal(_bits(_stack(outs, "dst_scale", n)), _bits(m.input2d("src_scale"))), f"{c.name}: the scales are not copies"


@pytest.mark.parametrize("case", fl.group("kv_copy"), ids=lambda c: c.name)
def test_kv_copy_spans(B, arena, case):
    run_case(B, arena, case, _launch_copy, _check_copy)


def test_kv_copy_spans_refuses_a_grid_it_cannot_launch(B, arena):
    """n_layers above the grid's y limit is refused by the argument check, and nothing is written: a refusal is a pass, a silent
    wrap is not."""
    c = fl.BY_NAME["kv_copy_spans_bf16_far_layer"]
    m = Mem(c, True, arena)
    src, dst = _copy_view(c, m, "src", fl.COPY_D), _copy_view(c, m, "dst", fl.COPY_D)
    many = lambda t: t.as_strided((65536,) + tuple(t.shape[1:]), (0,) + tuple(t.stride()[1:]))
    ids = torch.zeros(2, dtype=I32, device=DEV)
    with pytest.raises(B.IclError, match="grid too large"):
        B.kv_copy_spans(many(src), many(dst), 2, src_seq=ids, dst_seq=ids, n_fixed=fl.COPY_N)
    outs, bad = m.finish()
    assert not bad and all(bool(torch.isnan(v.float()).all()) for v in outs.values()), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# window-level Q-Former cross attention
# ------------------------------------------------------------------------------------------------------------------
def _launch_qformer(B, c, m):
    rpa = m.meta("kv", "rpa")
    kv = m.ptr("kv").as_strided((rpa + fl.QF_WIN, 128), (128, 1))
    B.qformer_window_xattn(m.rows2d("q"), kv, 64, m.rows2d("out"), 2, 1, fl.QF_WIN, rpa, c.p["H"], 0.125)


def _check_qformer(B, c, m, outs, aux):
    from oracle import attention as oa
    kv = m.input2d("kv").view(2 * fl.QF_WIN, 128)
    R = oa.qformer_ref(m.input2d("q"), kv, 64, 2, 1, fl.QF_WIN, fl.QF_WIN, c.p["H"], 0.125)
    oa.assert_bound(_stack(outs, "out", 2).view(2, c.p["H"], 64), R, 64, oa.R_P["qformer"], c.name)


@pytest.mark.parametrize("case", fl.group("qformer"), ids=lambda c: c.name)
def test_qformer_window_xattn(B, arena, case):
    run_case(B, arena, case, _launch_qformer, _check_qformer)


# ------------------------------------------------------------------------------------------------------------------
# prefill attention
# ------------------------------------------------------------------------------------------------------------------
def _launch_prefill(B, c, m):
    H, D = c.p["H"], c.p["D"]
    cu = torch.tensor([0, 1, 2], dtype=I32, device=DEV)
    kw = dict(causal=c.p["causal"])
    if c.p["suffix"]:
        kw["cu_q"] = cu.clone()             # every sequence keeps its one (last) query
    B.attn_fwd(m.rows2d("q"), m.rows2d("k"), m.rows2d("v"), m.rows2d("out"), cu, 1, H, D, D ** -0.5, **kw)


def _check_prefill(B, c, m, outs, aux):
    from oracle import attention as oa
    H, D = c.p["H"], c.p["D"]
    R = oa.prefill_ref(m.input2d("q"), m.input2d("k"), m.input2d("v"), [1, 1], H, D, D ** -0.5, causal=c.p["causal"])
    oa.assert_bound(_stack(outs, "out", 2).view(2, H, D), R, D, oa.R_P[f"prefill{D}"], c.name)


@pytest.mark.parametrize("case", fl.group("prefill"), ids=lambda c: c.name)
def test_prefill_attention_packed(B, arena, case):
    run_case(B, arena, case, _launch_prefill, _check_prefill)


def _prefill_rows(c):
    """(lengths of all sequences, packed q [total, H * D], packed row ranges of the checked sequences)."""
    from oracle import attention as oa
    lens = _grid_lens(c).tolist()
    cu = oa.cu_of(lens)
    q = torch.randn(cu[-1], c.p["H"] * c.p["D"], generator=_gen("prefill q", c.name)).to(BF16)
    rows = torch.cat([torch.arange(cu[s], cu[s + 1]) for s in fl.grid_checked(c.p["geom"])])
    return lens, cu, q, rows


def _launch_prefill_cache(B, c, m):
    # (the unchecked sequences read one position each of memory nobody initialised: their output rows are not compared)
    H, D = c.p["H"], c.p["D"]
    lens, cu, q, rows = _prefill_rows(c)
    q = q.to(DEV)
    out = torch.full_like(q, float("nan"))
    B.attn_fwd(q, m.ptr("kc"), m.ptr("vc"), out, torch.tensor(cu, dtype=I32, device=DEV), fl.GRID_ROWS, H, D, D ** -0.5,
               causal=c.p["causal"], kv_cache_max_len=m.meta("kc", "max_len"), n_kv_heads=c.p["Hkv"] if H != c.p["Hkv"] else 0)
    return dict(out=out[rows.to(DEV)])


def _check_prefill_cache(B, c, m, outs, aux):
    from oracle import attention as oa
    H, D = c.p["H"], c.p["D"]
    chk = fl.grid_checked(c.p["geom"])
    _, _, q, rows = _prefill_rows(c)
    lens = list(chk.values())
    pack = lambda nm: torch.cat([m.inputs[(nm, i)].view(fl.GRID_ROWS, 1, D)[:L].expand(L, H, D).reshape(L, H * D)
                                 for i, L in enumerate(lens)])             # query head h reads the one K/V head
    R = oa.prefill_ref(q[rows], pack("kc"), pack("vc"), lens, H, D, D ** -0.5, causal=c.p["causal"])
    oa.assert_bound(aux["out"].view(-1, H, D), R, D, oa.R_P[f"prefill{D}"], c.name)


@pytest.mark.parametrize("case", fl.group("prefill_cache"), ids=lambda c: c.name)
def test_prefill_attention_cache_layout(B, arena, case):
    run_case(B, arena, case, _launch_prefill_cache, _check_prefill_cache)


# ------------------------------------------------------------------------------------------------------------------
# the prompt-attention readout
# ------------------------------------------------------------------------------------------------------------------
def _segmass_near(c, grid):
    """The operands that stay near: (lens, q [n, H * D] or None, seg [n, width] or None, kc [2, 1, max_len, D] or None)."""
    g = _gen("segmass", c.name)
    if grid:
        lens = _grid_lens(c)
        q = torch.randn(len(lens), c.p["D"], generator=g).to(BF16)
        seg = torch.randint(0, fl.SM_NSEG + 1, (len(lens), fl.GRID_ROWS), generator=g).to(U8)      # id n_seg: counted nowhere
        return lens, q, seg, None
    kc = torch.randn(2, 1, fl.SM_MAXLEN, c.p["D"], generator=g).to(BF16)
    return torch.tensor(fl.SM_LENS, dtype=I32), None, None, kc


def _launch_segmass(B, c, m):
    D, H = c.p["D"], c.p["H"]
    grid = "geom" in c.p
    lens, q, seg, kc = _segmass_near(c, grid)
    mass = torch.full((len(lens), H, fl.SM_NSEG), float("nan"), dtype=F32, device=DEV)
    if grid:
        max_len = m.meta("kc", "max_len")
        segd = torch.zeros(len(lens), max_len, dtype=U8, device=DEV)
        segd[:, :fl.GRID_ROWS] = seg.to(DEV)
        B.attn_segmass(q.to(DEV), m.ptr("kc"), lens.to(DEV), segd, mass, H, D, max_len, D ** -0.5)
        return dict(mass=mass[torch.tensor(list(fl.grid_checked(c.p["geom"])), device=DEV)])
    rows = m.meta("q", "ids")
    qv = m.ptr("q").as_strided((max(rows) + 1, H * D), (H * D, 1))
    ld = m.meta("probs", "ld")
    probs = m.ptr("probs").as_strided((2, H, fl.SM_MAXLEN), (H * ld, ld, 1))
    B.attn_segmass(qv, kc.to(DEV), lens.to(DEV), m.rows2d("seg"), mass, H, D, fl.SM_MAXLEN, D ** -0.5,
                   q_rows=torch.tensor(rows, dtype=I32, device=DEV), probs=probs)
    return dict(mass=mass)


def _check_segmass(B, c, m, outs, aux):
    import attn_segmass_ref as sr
    D, H = c.p["D"], c.p["H"]
    grid = "geom" in c.p
    lens, q, seg, kc = _segmass_near(c, grid)
    if grid:
        chk = list(fl.grid_checked(c.p["geom"]))
        q, seg, lens = q[chk], seg[chk], lens[chk]
        kc = m.input2d("kc").view(len(chk), 1, fl.GRID_ROWS, D)
    else:
        q, seg = m.input2d("q"), m.input2d("seg")
    R = sr.reference(q, kc, lens.tolist(), seg, fl.SM_NSEG, H, 1, D, D ** -0.5)
    rm = sr.mass_ratio(aux["mass"], R, D)
    assert float(rm.max()) <= 1, f"{c.name}: mass err/bound {float(rm.max()):.3g} at {sr.describe(rm)}"
    if not grid:
        probs = _stack(outs, "probs", 2).view(2, H, fl.SM_MAXLEN)
        rp = sr.probs_ratio(probs, R, D)
        assert float(rp.max()) <= 1, f"{c.name}: probs err/bound {float(rp.max()):.3g} at {sr.describe(rp)}"
        assert bool(torch.isnan(probs[~R.live[:, None, :].expand_as(probs)]).all()), f"{c.name}: probs written at or past a length"


def _segmass_row_data(c, o, i):
    g = _gen(c.name, o.name, i)
    if o.dtype == "u8":
        return torch.randint(0, fl.SM_NSEG + 1, (o.n,), generator=g).to(U8)
    return torch.randn(o.n, generator=g).to(DT[o.dtype])


ROW_DATA["segmass"] = _segmass_row_data


@pytest.mark.parametrize("case", fl.group("segmass"), ids=lambda c: c.name)
def test_attn_segmass(B, arena, case):
    run_case(B, arena, case, _launch_segmass, _check_segmass)


# ------------------------------------------------------------------------------------------------------------------
# the audio front end
# ------------------------------------------------------------------------------------------------------------------
N_MEL, XT_LD = 80, 88


def _frontend_row_data(c, o, i):
    """A clip: noise of amplitude 0.1 up to its length, NaN in every sample the kernels may not read."""
    x = torch.full((o.n,), float("nan"))
    L = c.p["lens"][i]
    x[:L] = (torch.randn(L, generator=_gen(c.name, i)) * 0.1).clamp(-1, 1)
    return x


ROW_DATA["frontend"] = _frontend_row_data


def _launch_frontend(B, c, m):
    from oracle import audio_frontend as af
    wav = m.rows2d("wav")
    wl = torch.tensor(c.p["lens"], dtype=I32, device=DEV)
    if c.name == "logmel_whisper":
        T = af.N_FRAMES
        mel = torch.from_numpy(af.slaney_mel_filters(N_MEL)).to(DEV)
        spec = torch.full((2, N_MEL, T), float("nan"), dtype=F32, device=DEV)
        xt = torch.full((2, T + 2, XT_LD), float("nan"), dtype=BF16, device=DEV)
        B.logmel_whisper(wav, wl, mel, N_MEL, spec, xt, torch.empty(2 * N_MEL * T + 2, dtype=F32, device=DEV))
        return dict(spec=spec, xt=xt)
    frames = af.kaldi_num_frames(max(c.p["lens"]))
    out = torch.full((2, frames, 128), float("nan"), dtype=F32, device=DEV)
    B.fbank_kaldi(wav, wl, torch.from_numpy(af.kaldi_mel_banks()).to(DEV), frames, af.FBANK_MEAN, af.FBANK_STD, out)
    return dict(out=out)


def _check_frontend(B, c, m, outs, aux):
    import numpy as np
    import fp64_bounds as fb
    from oracle import audio_frontend as af
    for i, L in enumerate(c.p["lens"]):
        x = m.inputs[("wav", i)][:L].numpy()
        if c.name == "logmel_whisper":
            ref, e = fb.whisper_ref_bound(torch.from_numpy(af.whisper_logmel(x, N_MEL, as_f64=True)))
            fb.assert_within(aux["spec"][i], ref, e, f"{c.name} clip {i}")
        else:
            mean, std = float(np.float32(af.FBANK_MEAN)), float(np.float32(af.FBANK_STD))
            ref, e = fb.kaldi_ref_bound(torch.from_numpy(af.kaldi_fbank(x, mean, std, as_f64=True)))
            nf = af.kaldi_num_frames(L)
            assert ref.shape[0] == nf and bool(torch.isnan(aux["out"][i, nf:]).all())
            fb.assert_within(aux["out"][i, :nf], ref, e, f"{c.name} clip {i}")
    if c.name == "logmel_whisper":                                    # xt is the exact image of spec
        want = torch.zeros_like(aux["xt"])
        want[:, 1:-1, :N_MEL] = aux["spec"].transpose(1, 2).to(BF16)
        assert torch.equal(_bits(aux["xt"]), _bits(want)), f"{c.name}: xt is not the image of spec"


@pytest.mark.parametrize("case", fl.group("frontend"), ids=lambda c: c.name)
def test_audio_front_end(B, arena, case):
    run_case(B, arena, case, _launch_frontend, _check_frontend)


def test_logmel_refuses_a_far_xt_ld(B, arena):
    """xt_ld is bounded by the entry point ([n_mel, 128]): a far row stride of the log-mel output is refused, nothing is written."""
    from oracle import audio_frontend as af
    c = fl.BY_NAME["logmel_whisper"]
    m = Mem(c, True, arena)
    xt = m.ptr("wav").view(BF16).as_strided((2, 2, N_MEL), (0, fl.LD_FAR, 1))          # only its row stride reaches the entry point
    mel = torch.from_numpy(af.slaney_mel_filters(N_MEL)).to(DEV)
    with pytest.raises(B.IclError, match="xt_ld"):
        B.logmel_whisper(m.rows2d("wav"), torch.tensor(c.p["lens"], dtype=I32, device=DEV), mel, N_MEL, None, xt,
                         torch.empty(2 * N_MEL * af.N_FRAMES + 2, dtype=F32, device=DEV))
    _, bad = m.finish()
    assert not bad, "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# the QKV projection with RoPE + append fused into the 256x256 tile's epilogue
# ------------------------------------------------------------------------------------------------------------------
def _fused_gemm_args(c):
    import qknorm_ref as qr
    H, D, K = c.p["H"], c.p["D"], c.p["K"]
    g = _gen("gemm_rope w")
    w = (torch.randn(3 * H * D, K, generator=g) * 0.1).to(BF16)
    return H, D, H * D, w, torch.randn(3 * H * D, generator=g), qr.rope_tables(D, fl.ROPE_MAXLEN), torch.tensor(fl.ROPE_POS, dtype=I32)


def _launch_fused_gemm(B, c, m):
    H, D, hd, w, bias, (cos, sin), pos = _fused_gemm_args(c)
    w, bias, cos, sin, pos = dev(w, bias, cos, sin, pos)
    sid = torch.tensor(m.meta("kc", "ids"), dtype=I32, device=DEV)
    B.gemm(m.rows2d("a"), w, m.rows2d("c"), bias=bias, tile=3,
           rope=(hd, 2 * hd, cos, sin, pos, sid, m.ptr("kc"), m.ptr("vc"), H, D, fl.ROPE_MAXLEN))


def _check_fused_gemm(B, c, m, outs, aux):
    """The fused launch's contract (tests/test_gpu_kernels.py): bit-identical to icl_gemm_bf16 on the same tile followed by
    icl_rope_kv_bf16, each held to float64 by its own case above."""
    H, D, hd, w, bias, (cos, sin), pos = _fused_gemm_args(c)
    M = c.p["M"]
    w, bias, cos, sin, pos = dev(w, bias, cos, sin, pos)
    ref = torch.full((M, 3 * hd), float("nan"), dtype=BF16, device=DEV)
    B.gemm(m.input2d("a").to(DEV), w, ref, bias=bias, tile=3)
    kc = torch.full((M, H, fl.ROPE_MAXLEN, D), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    B.rope_kv(ref, hd, 2 * hd, cos, sin, pos, torch.arange(M, dtype=I32, device=DEV), kc, vc, H, D, fl.ROPE_MAXLEN)
    assert torch.equal(_bits(_stack(outs, "c", M)), _bits(ref.cpu())), f"{c.name}: C differs from gemm + rope_kv"
    p = pos.cpu().long()
    for nm, want in (("kc", kc), ("vc", vc)):
        rows = torch.stack([want[i, h, p[i]] for i in range(M) for h in range(H)]).cpu()
        assert torch.equal(_bits(_stack(outs, nm, M * H)), _bits(rows)), f"{c.name}: {nm} rows differ from gemm + rope_kv"
    assert not bool(torch.isnan(ref.float()).any())


@pytest.mark.parametrize("case", fl.group("gemm_rope"), ids=lambda c: c.name)
def test_gemm_rope_kv(B, arena, case):
    run_case(B, arena, case, _launch_fused_gemm, _check_fused_gemm)
