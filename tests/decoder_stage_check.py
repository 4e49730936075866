"""Teacher-forced, stage-by-stage check of the LLM decoder chain (LlamaHIP.embed / prefill / _last_layer_rows / decode_step / logits
of runtime/engines.py).  Not a test module and not a conftest: tests/test_gpu_decoder_stages.py runs it on the kernels,
tests/test_decoder_stages.py on the emulation of tests/decoder_emulation.py.

``recording()`` wraps every launching wrapper of runtime.binding the decoder uses.  Many decoder launches work in place (``h +=``,
the rotation inside ``qkv``, the cache append), so unlike the encoder's recorder it keeps a BEFORE and an AFTER copy of the whole
storage behind every written argument, and clones of the small index tensors (``pos`` / ``seq_ids`` / ``lens``) and of a fused
GEMM's activation, which later launches overwrite.

``walk_prefill`` / ``walk_decode_step`` first compare the kinds of the launches with what the chain is expected to issue
(``ChainChanged``: not a numeric failure), then judge every element each launch wrote against the float64 specification of that
stage (oracle/decoder_stages.py), computed from the state dict and the logical contents of the PREVIOUS stage's actual output.
The bounds are those the kernel families already have (tests/fp64_bounds.py, tests/qknorm_ref.py, oracle/attention.py): f32 GEMM
outputs gemm_ref_bound, bf16 ones + bf16_out_bound, SwiGLU swiglu_ref_bound, norms / LoRA down / RoPE / qk-norm as bf16 intervals,
attention err_bound with the kernel's r_P, data movers, FP8 bytes and scales bit for bit; a ``gemm_rmsnorm`` launch's C is held to
the GEMM bound and its ``xn`` to one bf16 ulp of the float64 RMSNorm of the kernel's own C row (tests/test_gpu_decode_plan.py).
After each launch, every element of the written storages OUTSIDE what the stage owns must be bit-identical to its before copy:
the LoRA columns and the zero tail under a fused norm, the k / v columns of ``pf_qkv`` under a cache-appending epilogue, every
other (layer, sequence, head, position) of every cache plane.

The three fused launch kinds (GEMM with the RoPE epilogue, attn_decode_rope, attn_decode_rope_fp8) promise the bits of their
two-launch form and hide their intermediate, so the walk replays the two-launch form on clones of the recorded before-state,
judges the replay per stage as above, and then requires the fused launch's outputs to be bit-identical to the replay's.

A miss raises ``StageFailure(stage, first element)``; ``Walk.worst`` holds the largest err / bound per stage kind."""
import contextlib
import functools
import inspect

import torch

import encoder_stage_check as esc
import fp64_bounds as fb
from encoder_stage_check import ChainChanged, StageFailure  # noqa: F401  (the callers' names for them)
from oracle import attention as oa
from oracle import decoder_stages as ds

BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
NAN = float("nan")

ROPE3 = ("qkv", "kcache", "vcache")
FP8_PLANES = ("kq", "vq", "ks", "vs")
WRITTEN = dict(embed_gather_interleave=("out",), rmsnorm=("out",), lora_down=("x",), gemm=("out",), gemm_rmsnorm=("out", "xn"),
               rope_kv=ROPE3, rope_kv_gqa=ROPE3, qknorm_rope_kv=ROPE3, rope_kv_fp8=("qkv",) + FP8_PLANES, kv_append_fp8=FP8_PLANES,
               attn_fwd=("out",), attn_decode=("out",), attn_decode_gqa=("out",), attn_decode_fp8=("out",),
               attn_decode_rope=("out", "qkv", "kcache", "vcache"), attn_decode_rope_fp8=("out", "qkv") + FP8_PLANES,
               gather_rows=("out",))


def _whole(t):
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Written:
    """Copies of the whole storage behind one written argument, before and after the launch, and the argument's geometry."""

    def __init__(self, t, before=None):
        self.shape, self.stride, self.offset = tuple(t.shape), tuple(t.stride()), t.storage_offset()
        self.storage = t.untyped_storage().data_ptr()
        self.before = _whole(t).clone() if before is None else before
        self.after = None

    def done(self, t):
        self.after = _whole(t).clone()

    def view(self, before=False):
        """What the argument showed after (before) the launch."""
        return torch.as_strided(self.before if before else self.after, self.shape, self.stride, self.offset)

    def like(self, t, before=False):
        """The copy seen through the geometry of ``t``, a tensor (or another Written) over the same storage."""
        g = (t.shape, t.stride, t.offset) if isinstance(t, Written) else (tuple(t.shape), tuple(t.stride()), t.storage_offset())
        return torch.as_strided(self.before if before else self.after, *g)

    def replay(self, shared):
        """(a live tensor with the argument's geometry over a clone of the before copy, the Written that will hold the result).
        ``shared``: the clones of one replay by storage, so that two arguments over one storage stay aliased in the replay."""
        flat = shared.setdefault(self.storage, self.before.clone())
        r = Written.__new__(Written)
        r.shape, r.stride, r.offset, r.before, r.after = self.shape, self.stride, self.offset, self.before, flat
        return torch.as_strided(flat, self.shape, self.stride, self.offset), r


class Launch:
    def __init__(self, name, written, args, ints, act):
        self.name, self.written, self.args, self.ints, self.act = name, written, args, ints, act

    def __getitem__(self, arg):
        return self.written[arg]


class Launches(list):
    fns = None          # name -> the wrapper underneath the recorder (the kernel's, or its emulation): what a replay calls


def _targets(name, a):
    t = {k: a[k] for k in WRITTEN[name] if a.get(k) is not None}
    if name == "gemm" and a.get("rope") is not None:
        for k, v in (("kcache", a["rope"][6]), ("vcache", a["rope"][7])):
            if v is not None:
                t[k] = v
    return t


@contextlib.contextmanager
def recording(mutate=None):
    """-> the ``Launches`` list, appended to as the decoder wrappers of runtime.binding are called.  ``mutate(name, ordinal,
    arguments)`` (optional; ordinal counts the launches of that wrapper in this recording) may alter the bound arguments of a
    launch before anything is copied or launched, or return "skip" to leave the launch out: a planted host-side mistake, seen by
    the recorder exactly as the host code would have made it."""
    import icl_speech_text_llm_amd.runtime.binding as B
    saved = {n: getattr(B, n) for n in WRITTEN}
    launches = Launches()
    launches.fns = {n: getattr(f, "__wrapped__", f) for n, f in saved.items()}
    counts = {n: 0 for n in saved}

    def wrapper(name, f):
        sig = inspect.signature(f)

        @functools.wraps(f)
        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            counts[name] += 1
            skip = mutate is not None and mutate(name, counts[name] - 1, a) == "skip"
            targets = _targets(name, a)
            wr = {k: Written(t) for k, t in targets.items()}
            pool = dict(a)
            if a.get("rope") is not None:
                pool.update(pos=a["rope"][4], seq_ids=a["rope"][5])
            ints = {k: v.clone() for k, v in pool.items() if isinstance(v, torch.Tensor) and v.dtype == I32}
            act = a["a"].clone() if a.get("rope") is not None else None
            r = a.get("out") if skip else f(**a)
            for k, t in targets.items():
                wr[k].done(t)
            launches.append(Launch(name, wr, a, ints, act))
            return r
        call.__wrapped__ = getattr(f, "__wrapped__", f)
        return call

    try:
        for n, f in saved.items():
            setattr(B, n, wrapper(n, f))
        yield launches
    finally:
        for n, f in saved.items():
            setattr(B, n, f)


# ---------------------------------------------------------------------------------------------------------------------------
# the walker
# ---------------------------------------------------------------------------------------------------------------------------
class Walk(esc.Walk):
    def __init__(self, launches, expected):
        super().__init__(launches, expected)
        self.fns = launches.fns

    def exact(self, stage, got, want):
        assert got.dtype == want.dtype and got.shape == want.shape, (stage, got.dtype, want.dtype, got.shape, want.shape)
        self.worst.setdefault("exact", 0.0)
        bad = _bits(got) != _bits(want.to(got.device))
        if bool(bad.any()):
            self.worst["exact"] = float("inf")
            raise StageFailure(stage, f"{int(bad.sum())} of {bad.numel()} elements differ from the exact image, first at "
                                      f"{bad.nonzero()[0].tolist()}")

    def rest(self, stage, wr, *views):
        """Everything of the written storage outside ``views`` (views of ``wr.after``) is bit-identical to the before copy."""
        want = wr.before.clone()
        for v in views:
            torch.as_strided(want, v.shape, v.stride(), v.storage_offset()).copy_(v)
        self.exact(stage + ".rest", wr.after, want)

    def swiglu(self, stage, got, ref, e):
        e = fb.bf16_out_bound(e, ref, got)
        self._note(stage, "swiglu", fb.worst_ratio(got, ref, e), ~fb.within(got, ref, e))

    def ulp1(self, stage, got, c_row, gamma, eps):
        """xn of a gemm_rmsnorm launch: within 1 bf16 ulp of the float64 RMSNorm of the kernel's own C row."""
        c = c_row.double()
        xr = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps) * gamma.double()
        e = fb.bf16_ulp(torch.maximum(xr.abs(), got.double().abs()))
        self._note(stage, "fused_norm", fb.worst_ratio(got, xr, e), ~fb.within(got, xr, e))


def report(case, worst):
    for kind in sorted(worst):
        print(f"err/bound decoder stages {case} {kind}: {worst[kind]:.3f}")


class Ctx:
    """What every stage of one walk needs: the walk, the state dict and its prefix, the configuration, the FULL KV cache the test
    made (its planes give the geometry the copies are read through) and the first sequence of the chunk the call ran on."""

    def __init__(self, w, sd, prefix, cfg, cache=None, b0=0):
        self.w, self.sd, self.prefix, self.cfg, self.cache, self.b0 = w, sd, prefix, cfg, cache, b0
        self.fp8 = cache is not None and cache.dtype == "fp8"
        self.k_off, self.v_off = cfg.n_heads * cfg.head_dim, (cfg.n_heads + cfg.kv_heads) * cfg.head_dim
        self.r2 = cfg.lora_rank * len(cfg.lora_targets) if cfg.lora_rank else 0


# ---------------------------------------------------------------------------------------------------------------------------
# expected launches
# ---------------------------------------------------------------------------------------------------------------------------
def _head_kinds(cfg, decode, M, ready):
    return ([] if ready else ["rmsnorm"]) + ([("lora_down" if decode and M > 64 else "gemm")] if cfg.lora_rank else [])


def prefill_kinds(cfg, M, form, embed=True, logits=False):
    """form: epilogue (the QKV GEMM carries the RoPE epilogue), trim (the last layer runs on the gathered rows), last_rows_only,
    fp8 (an FP8 KV cache)."""
    out = ["embed_gather_interleave"] if embed else []
    tail = ["gemm", "rmsnorm", "gemm", "gemm"]
    for i in range(cfg.n_layers):
        out += _head_kinds(cfg, False, M, False)
        if form["trim"] and i == cfg.n_layers - 1:
            out += ["gemm", "gather_rows", "gather_rows", "gemm", "attn_fwd"] + tail
            break
        out += ["gemm"]
        if not form["epilogue"]:
            out += ["qknorm_rope_kv" if cfg.qk_norm else "rope_kv_gqa" if cfg.group > 1 else "rope_kv"]
        out += (["kv_append_fp8"] if form["fp8"] else []) + ["attn_fwd"] + tail
    else:
        out += ["gather_rows"] if form["last_rows_only"] else []
    return out + (["rmsnorm", "gemm"] if logits else [])


def decode_kinds(cfg, Bn, fp8, fuse_rope, fuse_norms):
    out, ready = ["embed_gather_interleave"], False
    fuse_rope = fuse_rope and Bn > 8 and not cfg.qk_norm
    for _ in range(cfg.n_layers):
        out += _head_kinds(cfg, True, Bn, ready) + ["gemm"]
        if cfg.qk_norm:
            out += ["qknorm_rope_kv", "attn_decode_gqa" if cfg.group > 1 else "attn_decode"]
        elif cfg.group > 1:
            out += ["rope_kv_gqa", "attn_decode_gqa"]
        elif fp8:
            out += ["attn_decode_rope_fp8"] if fuse_rope else ["rope_kv_fp8", "attn_decode_fp8"]
        else:
            out += ["attn_decode_rope"] if fuse_rope else ["rope_kv", "attn_decode"]
        out += ["gemm_rmsnorm", "gemm", "gemm_rmsnorm"] if fuse_norms else ["gemm", "rmsnorm", "gemm", "gemm"]
        ready = fuse_norms
    return out + ([] if ready else ["rmsnorm"]) + ["gemm"]


# ---------------------------------------------------------------------------------------------------------------------------
# the stages of a layer
# ---------------------------------------------------------------------------------------------------------------------------
def _layer_input(C, st, lp, h, decode, ready):
    """The layer's input for the QKV projection -> (xn [M, hidden], t [M, LoRA columns] or None).  ``ready``: None, or
    (xn as the previous down launch's fused norm left it, the Written of that buffer)."""
    w, cfg = C.w, C.cfg
    hd, M = cfg.hidden, h.shape[0]
    if ready is None:
        buf = w.take("rmsnorm")["out"]
        xn = buf.view()[:, :hd]
        w.interval(st + "input_norm", "norm", xn, *ds.rms_norm(C.sd, lp + "input_layernorm.weight", h, cfg.rms_eps))
        w.rest(st + "input_norm", buf, xn)
    else:
        xn, buf = ready
    if not cfg.lora_rank:
        return xn, None
    dot, mag = ds.lora_down(C.sd, lp, cfg, xn)
    if decode and M > 64:
        wr = w.take("lora_down")["x"]
        full = wr.view()
        t = full[:, hd:hd + C.r2]
        w.interval(st + "lora_down", "lora", t, *fb.lora_ref_bound(xn, ds.lora_weight(C.sd, lp, cfg, xn.device), 1.0))
    else:
        wr = w.take("gemm")["out"]
        full = wr.like(buf)
        t = full[:, hd:hd + C.r2]
        w.gemm_bf16(st + "lora_down", t, *fb.gemm_ref_bound(dot, mag, hd))
    w.rest(st + "lora_down", wr, t)
    if tuple(full.shape) != (M, ds.k_aug(cfg)):
        raise StageFailure(st + "xn_tail", f"the layer's input buffer is {tuple(full.shape)}, not [{M}, {ds.k_aug(cfg)}]")
    w.exact(st + "xn_tail", full[:, hd + C.r2:], torch.zeros_like(full[:, hd + C.r2:]))     # the zero tail of the augmentation
    return xn, t


def _qkv_plain(C, st, lp, xn, t):
    wr = C.w.take("gemm")["out"]
    qkv = wr.view()
    C.w.gemm_bf16(st + "qkv", qkv, *ds.qkv(C.sd, lp, C.cfg, xn, t))
    C.w.rest(st + "qkv", wr, qkv)
    return qkv


def _judge_rotation(C, st, lp, before, after, positions, parts=("q", "k")):
    """before / after [M, q | k | v columns] bf16: the q and k blocks rotated at each row's position (behind the per-head norm of a
    QK-norm decoder).  The caller checks what else may have changed."""
    cfg, D = C.cfg, C.cfg.head_dim
    M = before.shape[0]
    blocks = dict(q=(0, C.k_off, "self_attn.q_norm.weight"), k=(C.k_off, C.v_off, "self_attn.k_norm.weight"))
    for name in parts:
        c0, c1, gain = blocks[name]
        x = before[:, c0:c1].reshape(M, -1, D)
        ref, e = ds.head_norm_rope(C.sd, lp + gain, cfg, x, positions) if cfg.qk_norm else ds.rope(cfg, x, positions)
        C.w.interval(st + "rope_" + name, "qknorm_rope" if cfg.qk_norm else "rope", after[:, c0:c1].reshape(M, -1, D), ref, e)


def _planes(C):
    c = C.cache
    return (("k", "kq" if C.fp8 else "kcache", c.k, "ks", c.ks), ("v", "vq" if C.fp8 else "vcache", c.v, "vs", c.vs))


def _judge_append(C, st, layer, written, k_rows, v_rows, seqs, positions):
    """The cache after an appending launch: rows (layer, sequence, head, position) hold k_rows / v_rows [M, Hkv, D] bit for bit
    (an FP8 cache: their e4m3 bytes and scales); every other element of every plane, in every layer, is bit-unchanged."""
    w, dev = C.w, k_rows.device
    s = (torch.as_tensor(seqs) + C.b0).to(dev)[:, None]
    p = torch.as_tensor(positions).to(dev)[:, None]
    hh = torch.arange(C.cfg.kv_heads, device=dev)[None]
    for (name, arg, plane, sarg, splane), rows in zip(_planes(C), (k_rows, v_rows)):
        wants = [(arg, plane, rows)]
        if C.fp8:
            b, sc, _ = ds.fp8_row(rows)
            wants = [(arg, plane, b), (sarg, splane, sc)]
        for a, pl, want in wants:
            wr = written[a]
            got = wr.like(pl)[layer, s, hh, p]
            w.exact(f"{st}cache_{name}" + ("" if a == arg else "_scale"), got, want)
            rest = wr.before.clone()
            torch.as_strided(rest, tuple(pl.shape), tuple(pl.stride()), pl.storage_offset())[layer, s, hh, p] = got
            w.exact(f"{st}cache_{name}" + ("" if a == arg else "_scale") + ".rest", wr.after, rest)


def _cached(C, layer, written, lens, seqs):
    """(keys, values) per row from the cache copies AFTER a launch: [Hkv, len, D] of (layer, sequence), dequantised if FP8."""
    out = []
    for name, arg, plane, sarg, splane in _planes(C):
        full = written[arg].like(plane)
        rows = [full[layer, s + C.b0, :, :n] for s, n in zip(seqs, lens)]
        if C.fp8:
            sc = written[sarg].like(splane)
            rows = [ds.dequant(r, sc[layer, s + C.b0, :, :n]) for r, s, n in zip(rows, seqs, lens)]
        out.append(rows)
    return out


def _attn_out_mlp(C, st, lp, h, att, fuse, next_gain):
    """From the attention output to the end of the layer -> (h, (xn of the next norm, its Written) or None)."""
    w, cfg, sd = C.w, C.cfg, C.sd
    hd = cfg.hidden
    if fuse:
        l = w.take("gemm_rmsnorm")
        h2, xbuf = l["out"].view(), l["xn"]
        xn = xbuf.view()[:, :hd]
        w.f32(st + "o_proj", "gemm", h2, *ds.linear(sd, lp + "self_attn.o_proj", att, residual=h))
        w.ulp1(st + "post_norm", xn, h2, ds._p(sd, lp + "post_attention_layernorm.weight", h2.device), cfg.rms_eps)
        w.rest(st + "o_proj", l["out"], h2)
        w.rest(st + "post_norm", xbuf, xn)
    else:
        wr = w.take("gemm")["out"]
        h2 = wr.view()
        w.f32(st + "o_proj", "gemm", h2, *ds.linear(sd, lp + "self_attn.o_proj", att, residual=h))
        w.rest(st + "o_proj", wr, h2)
        xbuf = w.take("rmsnorm")["out"]
        xn = xbuf.view()[:, :hd]
        w.interval(st + "post_norm", "norm", xn, *ds.rms_norm(sd, lp + "post_attention_layernorm.weight", h2, cfg.rms_eps))
        w.rest(st + "post_norm", xbuf, xn)
    wr = w.take("gemm")["out"]
    act = wr.view()
    w.swiglu(st + "gate_up", act, *ds.swiglu(sd, lp, xn))
    w.rest(st + "gate_up", wr, act)
    if fuse and next_gain is not None:
        l = w.take("gemm_rmsnorm")
        h3, nbuf = l["out"].view(), l["xn"]
        nxt = nbuf.view()[:, :hd]
        w.f32(st + "down", "gemm", h3, *ds.linear(sd, lp + "mlp.down_proj", act, residual=h2))
        w.ulp1(st + "next_norm", nxt, h3, ds._p(sd, next_gain, h3.device), cfg.rms_eps)
        w.rest(st + "down", l["out"], h3)
        w.rest(st + "next_norm", nbuf, nxt)
        return h3, (nxt, nbuf)
    wr = w.take("gemm")["out"]
    h3 = wr.view()
    w.f32(st + "down", "gemm", h3, *ds.linear(sd, lp + "mlp.down_proj", act, residual=h2))
    w.rest(st + "down", wr, h3)
    return h3, None


def _logits(C, h, ready, result):
    w, sd, p = C.w, C.sd, C.prefix
    if ready is None:
        buf = w.take("rmsnorm")["out"]
        xn = buf.view()
        w.interval("final_norm", "norm", xn, *ds.rms_norm(sd, p + "model.norm.weight", h, C.cfg.rms_eps))
        w.rest("final_norm", buf, xn)
    else:
        xn = ready[0]
    wr = w.take("gemm")["out"]
    out = wr.view()
    w.f32("lm_head", "gemm", out, *ds.linear(sd, p + "lm_head", xn))
    w.rest("lm_head", wr, out)
    if result is not None:
        w.exact("logits.result", result, out)


# ---------------------------------------------------------------------------------------------------------------------------
# the fused launches: the two-launch form replayed on the recorded before-state, judged, and compared bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def _gemm_rope(C, st, lp, layer, xn, t, which, positions, seqs):
    """A QKV GEMM with the RoPE epilogue over the projections ``which`` -> (the q block as the fused launch left it or None, the
    launch).  Replay: the plain GEMM on tile 3 into a bf16 C of its own, then icl_rope_kv_bf16 on full q | k | v rows holding it."""
    w, cfg, dev = C.w, C.cfg, xn.device
    l = w.take("gemm")
    a, rope = l.args, l.args["rope"]
    if rope is None:
        raise StageFailure(st + "qkv", "the QKV projection was expected to carry the RoPE epilogue")
    k_off, v_off, H, D, max_len = rope[0], rope[1], rope[8], rope[9], rope[10]
    to_c = bool(rope[11]) if len(rope) > 11 else True
    M, hd = xn.shape[0], H * D
    N = a["w"].shape[0] if a["N"] is None else a["N"]
    c = torch.full((M, N), NAN, dtype=BF16, device=dev)
    w.fns["gemm"](l.act, a["w"], c, bias=a["bias"], tile=3)
    w.gemm_bf16(st + "qkv", c, *ds.qkv(C.sd, lp, cfg, xn, t, which=which))
    full = torch.zeros(M, 3 * hd, dtype=BF16, device=dev)
    shift = hd - k_off                                         # where C's first column sits in a full row
    full[:, shift:shift + N] = c
    before = full.clone()
    caches, rep, shared = {}, {}, {}
    for k in ("kcache", "vcache"):
        if k in l.written:
            caches[k], rep[k] = l[k].replay(shared)
    w.fns["rope_kv"](full, hd, 2 * hd, rope[2], rope[3], l.ints["pos"], l.ints.get("seq_ids"), caches.get("kcache"),
                     caches.get("vcache"), H, D, max_len)
    parts = tuple(n[0] for n in which if n != "v_proj")
    _judge_rotation(C, st, lp, before, full, positions, parts)
    if "v_proj" in which:           # (the blocks the launch does not project are the replay's own zeros: not judged)
        w.exact(st + "rope.rest", full[:, 2 * hd:], before[:, 2 * hd:])
    if rep:
        _judge_append(C, st, layer, rep, full[:, hd:2 * hd].reshape(M, H, D), full[:, 2 * hd:].reshape(M, H, D), seqs, positions)
    # fused == replay
    out = l["out"]
    cols = N if to_c else k_off
    got = out.view()[:, :cols]
    w.exact(st + "fused.qkv", got, full[:, shift:shift + cols])
    w.rest(st + "fused.qkv", out, got)
    for k in rep:
        w.exact(st + "fused." + k, l[k].after, rep[k].after)
    return (got[:, :k_off] if k_off else None), l


def _decode_attention(C, st, layer, q, written, lens, got, r_p=None):
    keys, values = _cached(C, layer, written, lens, range(len(lens)))
    R = ds.cached_attention(q, keys, values, C.cfg)
    C.w.attention(st + "attn", "decode_attention", got, R, C.cfg.head_dim, oa.R_P["decode"] if r_p is None else r_p)


def _decode_rope_fused(C, st, lp, layer, positions, lens):
    """attn_decode_rope / attn_decode_rope_fp8 -> the attention output.  Replay: rope_kv(_fp8) then attn_decode(_fp8)."""
    w, cfg = C.w, C.cfg
    l = w.take("attn_decode_rope_fp8" if C.fp8 else "attn_decode_rope")
    a = l.args
    H, D, max_len = a["n_heads"], a["head_dim"], a["max_len"]
    before = l["qkv"].view(before=True)
    qkv = before.clone()
    names = FP8_PLANES if C.fp8 else ("kcache", "vcache")
    live, rep, shared = {}, {}, {}
    for k in names:
        live[k], rep[k] = l[k].replay(shared)
    w.fns["rope_kv_fp8" if C.fp8 else "rope_kv"](qkv, a["k_off"], a["v_off"], a["cos"], a["sin"], l.ints["pos"], l.ints["seq_ids"],
                                                  *[live[k] for k in names], H, D, max_len)
    M = qkv.shape[0]
    _judge_rotation(C, st, lp, before, qkv, positions, ("q",) if C.fp8 else ("q", "k"))
    k_rot = qkv[:, C.k_off:C.v_off]
    if C.fp8:       # the k block stays as projected; the cache holds the rounding of the bf16 rotation icl_rope_kv_bf16 gives
        ref, e = ds.rope(cfg, before[:, C.k_off:C.v_off].reshape(M, -1, D), positions)
        k_rot = _fp8_rotated_k(C, st, layer, rep, ref, e, positions)
        C.w.exact(st + "rope.rest", qkv[:, C.k_off:], before[:, C.k_off:])
    else:
        C.w.exact(st + "rope.rest", qkv[:, C.v_off:], before[:, C.v_off:])
    _judge_append(C, st, layer, rep, k_rot.reshape(M, -1, D), qkv[:, C.v_off:].reshape(M, -1, D), range(M), positions)
    att = torch.full((M, H * D), NAN, dtype=BF16, device=qkv.device)
    w.fns["attn_decode_fp8" if C.fp8 else "attn_decode"](qkv[:, :a["k_off"]], *[live[k] for k in names], att, l.ints["lens"], H, D,
                                                        max_len, a["scale"])
    _decode_attention(C, st, layer, qkv[:, :C.k_off], rep, lens, att)
    out = l["out"]
    w.exact(st + "fused.attn", out.view(), att)
    w.rest(st + "fused.attn", out, out.view())
    w.exact(st + "fused.qkv_unchanged", l["qkv"].after, l["qkv"].before)
    for k in names:
        w.exact(st + "fused." + k, l[k].after, rep[k].after)
    return out.view()


def _fp8_rotated_k(C, st, layer, written, ref, e, positions):
    """An FP8 append of a rotated k the launch does not leave anywhere in bf16: the bf16 rotation is any value of the rotation's
    interval; where the interval is one value (almost everywhere) that is the row.  -> the k rows [M, Hkv, D] bf16 the bytes must
    be the rounding of, after checking every candidate element against the interval."""
    lo, hi = fb.bf16_interval(ref, e)
    M = ref.shape[0]
    dev = ref.device
    kq, ks = written["kq"].like(C.cache.k), written["ks"].like(C.cache.ks)
    s = (torch.arange(M, device=dev) + C.b0)[:, None]
    p = torch.as_tensor(positions).to(dev)[:, None]
    hh = torch.arange(C.cfg.kv_heads, device=dev)[None]
    deq = ds.dequant(kq[layer, s, hh, p], ks[layer, s, hh, p])            # what the cache row stands for
    # a one-value interval pins the element; elsewhere take the end of the interval nearer to the stored value
    pick = torch.where((deq - lo).abs() <= (deq - hi).abs(), lo, hi)
    return pick.to(BF16)


# ---------------------------------------------------------------------------------------------------------------------------
# the chains
# ---------------------------------------------------------------------------------------------------------------------------
def _embed(C, src, speech):
    wr = C.w.take("embed_gather_interleave")["out"]
    h = wr.view()
    C.w.exact("embed", h, ds.embed(C.sd, C.prefix, src, speech, h.device))
    C.w.rest("embed", wr, h)
    return h


def _packed_from_cache(keys, lens):
    """[Hkv, len, D] per sequence -> the packed rows [sum lens, Hkv D]."""
    return torch.cat([k.transpose(0, 1).reshape(n, -1) for k, n in zip(keys, lens)])


def walk_prefill(launches, sd, prefix, cfg, src, speech, seq_lens, form, result, *, cache=None, b0=0, h_in=None, logits=None):
    """One ``embed`` + ``prefill`` (+ ``logits``) of LlamaHIP over the packed rows ``src`` (token ids; -1 - j: speech row j) of
    sequences of ``seq_lens`` positions.  ``cache``: the whole KVCache the test made, of which the call was given sequences
    b0 .. b0 + len(seq_lens) - 1 (``KVCache.rows``); ``h_in``: the rows given to prefill when the embedding was not part of the
    recording (a chunk of an earlier embed); ``result``: what prefill returned; ``logits``: None, or what logits returned."""
    M, n = sum(seq_lens), len(seq_lens)
    w = Walk(launches, prefill_kinds(cfg, M, form, embed=h_in is None, logits=logits is not None))
    C = Ctx(w, sd, prefix, cfg, cache, b0)
    D, hd, Hkv = cfg.head_dim, cfg.hidden, cfg.kv_heads
    positions = [p for s in seq_lens for p in range(s)]
    seqs = [b for b, s in enumerate(seq_lens) for _ in range(s)]
    last = [e - 1 for e in oa.cu_of(seq_lens)[1:]]
    h = _embed(C, src, speech) if h_in is None else h_in
    r_p = oa.R_P[f"prefill{D}"]
    final = None
    for i in range(cfg.n_layers):
        lp, st = ds.layer_prefix(prefix, i), f"L{i}."
        xn, t = _layer_input(C, st, lp, h, False, None)
        if form["trim"] and i == cfg.n_layers - 1:
            _, l = _gemm_rope(C, st + "kv.", lp, i, xn, t, ("k_proj", "v_proj"), positions, seqs)
            if "out" in l.written and not ds.same_bits(l["out"].after, l["out"].before):
                raise StageFailure(st + "kv.fused.qkv", "the k | v launch of the trimmed layer wrote its C")
            wr = w.take("gather_rows")["out"]
            hg = wr.view()
            w.exact(st + "gather_h", hg, h[last])
            w.rest(st + "gather_h", wr, hg)
            wr = w.take("gather_rows")["out"]
            xg = wr.view()
            w.exact(st + "gather_xn", xg[:, :hd], xn[last])
            if t is not None:
                w.exact(st + "gather_xn.lora", xg[:, hd:hd + C.r2], t[last])
            w.exact(st + "gather_xn.tail", xg[:, hd + C.r2:], torch.zeros_like(xg[:, hd + C.r2:]))
            w.rest(st + "gather_xn", wr, xg)
            q, l = _gemm_rope(C, st + "q.", lp, i, xn[last], None if t is None else t[last], ("q_proj",),
                              [s - 1 for s in seq_lens], list(range(n)))
            la = w.take("attn_fwd")
            keys, values = _cached(C, i, _cache_copies(C, la, launches), seq_lens, range(n))
            att = la["out"].view()
            w.attention(st + "attn", "attention", att, ds.cached_attention(q, keys, values, cfg), D, r_p)
            w.rest(st + "attn", la["out"], att)
            final, _ = _attn_out_mlp(C, st, lp, hg, att, False, None)
            break
        if form["epilogue"]:
            to_cache = cache is not None and not C.fp8
            q, l = _gemm_rope(C, st, lp, i, xn, t, ds.PROJ, positions, seqs)
            qkv = l["out"].view()
            if to_cache:          # k / v are in the cache only: the attention reads them there
                keys, values = _cached(C, i, l.written, seq_lens, range(n))
                k_rot, v = _packed_from_cache(keys, seq_lens), _packed_from_cache(values, seq_lens)
            else:
                k_rot, v = qkv[:, C.k_off:C.v_off], qkv[:, C.v_off:]
        else:
            before = _qkv_plain(C, st, lp, xn, t)
            l = w.take("qknorm_rope_kv" if cfg.qk_norm else "rope_kv_gqa" if cfg.group > 1 else "rope_kv")
            qkv = l["qkv"].view()
            _judge_rotation(C, st, lp, before, qkv, positions)
            w.rest(st + "rope", l["qkv"], qkv[:, :C.v_off])
            q, k_rot, v = qkv[:, :C.k_off], qkv[:, C.k_off:C.v_off], qkv[:, C.v_off:]
            if cache is not None and not C.fp8:
                _judge_append(C, st, i, l.written, k_rot.reshape(M, Hkv, D), v.reshape(M, Hkv, D), seqs, positions)
            elif "kcache" in l.written or "vcache" in l.written:
                raise StageFailure(st + "rope", "a cache was handed to a RoPE launch that must append nowhere")
        if C.fp8:
            l = w.take("kv_append_fp8")
            _judge_append(C, st, i, l.written, k_rot.reshape(M, Hkv, D), v.reshape(M, Hkv, D), seqs, positions)
        la = w.take("attn_fwd")
        att = la["out"].view()
        w.attention(st + "attn", "attention", att, ds.causal_attention(q, k_rot, v, seq_lens, cfg), D, r_p)
        w.rest(st + "attn", la["out"], att)
        h, _ = _attn_out_mlp(C, st, lp, h, att, False, None)
    else:
        final = h
        if form["last_rows_only"]:
            wr = w.take("gather_rows")["out"]
            final = wr.view()
            w.exact("gather_last", final, h[last])
            w.rest("gather_last", wr, final)
    w.exact("prefill.result", result, final)
    if logits is not None:
        _logits(C, final, None, logits)
    w.done()
    return w.worst


def _cache_copies(C, la, launches):
    """The cache as the suffix attention of the trimmed layer saw it: the after copies of the last launch before it that wrote
    the planes (the k | v GEMM of that layer)."""
    k = launches.index(la)
    for l in reversed(launches[:k]):
        if "kcache" in l.written:
            return l.written
    raise StageFailure("attn", "no launch before the suffix attention wrote the cache")


def walk_decode_step(launches, sd, prefix, cfg, ids, positions, cache, result, *, fuse_rope=True, fuse_norms=True):
    """One ``decode_step`` of LlamaHIP: row b feeds token ``ids[b]`` at position ``positions[b]`` of sequence b of ``cache`` and
    attends positions 0 .. positions[b]."""
    Bn = len(ids)
    w = Walk(launches, decode_kinds(cfg, Bn, cache.dtype == "fp8", fuse_rope, fuse_norms))
    C = Ctx(w, sd, prefix, cfg, cache, 0)
    D, Hkv = cfg.head_dim, cfg.kv_heads
    lens = [p + 1 for p in positions]
    fused_rope = fuse_rope and Bn > 8 and not cfg.qk_norm and cfg.group == 1
    h = _embed(C, list(ids), None)
    ready = None
    for i in range(cfg.n_layers):
        lp, st = ds.layer_prefix(prefix, i), f"L{i}."
        xn, t = _layer_input(C, st, lp, h, True, ready)
        before = _qkv_plain(C, st, lp, xn, t)
        if fused_rope:
            att = _decode_rope_fused(C, st, lp, i, positions, lens)
        else:
            l = w.take("qknorm_rope_kv" if cfg.qk_norm else "rope_kv_gqa" if cfg.group > 1 else "rope_kv_fp8" if C.fp8 else "rope_kv")
            qkv = l["qkv"].view()
            _judge_rotation(C, st, lp, before, qkv, positions, ("q",) if C.fp8 else ("q", "k"))
            w.rest(st + "rope", l["qkv"], qkv[:, :C.k_off] if C.fp8 else qkv[:, :C.v_off])
            k_rot = qkv[:, C.k_off:C.v_off].reshape(Bn, Hkv, D)
            if C.fp8:
                k_rot = _fp8_rotated_k(C, st, i, l.written, *ds.rope(cfg, before[:, C.k_off:C.v_off].reshape(Bn, Hkv, D), positions),
                                       positions)
            _judge_append(C, st, i, l.written, k_rot, qkv[:, C.v_off:].reshape(Bn, Hkv, D), range(Bn), positions)
            la = w.take("attn_decode_gqa" if cfg.group > 1 else "attn_decode_fp8" if C.fp8 else "attn_decode")
            att = la["out"].view()
            _decode_attention(C, st, i, qkv[:, :C.k_off], l.written, lens, att)
            w.rest(st + "attn", la["out"], att)
        nxt = ds.layer_prefix(prefix, i + 1) + "input_layernorm.weight" if i + 1 < cfg.n_layers else prefix + "model.norm.weight"
        h, ready = _attn_out_mlp(C, st, lp, h, att, fuse_norms, nxt)
    _logits(C, h, ready, result)
    w.done()
    return w.worst


# ---------------------------------------------------------------------------------------------------------------------------
# runtimes and buffers for the tests
# ---------------------------------------------------------------------------------------------------------------------------
def cpu_llama(cfg, sd, prefix="llama_model.", weight_dtype="bf16", **switches):
    """A LlamaHIP on CPU tensors (the constructor insists on a GPU); call inside ``decoder_emulation.installed()``."""
    from icl_speech_text_llm_amd.runtime import engines as E, packing as P
    rt = object.__new__(E.LlamaHIP)
    rt.w, rt.device, rt.n_cu, rt.weight_dtype = P.pack_llama(dict(sd), cfg, "cpu", prefix=prefix), torch.device("cpu"), 256, weight_dtype
    for k, v in switches.items():
        setattr(rt, k, v)
    if weight_dtype == "fp8":
        rt._quantize_fp8()
    return rt


def poison_cache(cache):
    """NaN in every element of every plane (an FP8 byte 0x7f is NaN): a read past ``lens`` or of a stale row shows."""
    for t in (cache.k, cache.v):
        t.fill_(0x7F if t.dtype == U8 else NAN)
    for t in (cache.ks, cache.vs):
        if t is not None:
            t.fill_(NAN)


def poison_workspace(ws, cfg, rows, seqs):
    """NaN in the never-zeroed buffers of a prefill over ``rows`` packed rows of ``seqs`` sequences and of a decode step over
    ``seqs`` rows, written through the tensors Workspace.get returns (the zero=True buffers pf_xn / dc_xn keep their contract)."""
    W, hd, I = ds.proj_rows(cfg)["v_proj"][0] + ds.proj_rows(cfg)["v_proj"][1], cfg.hidden, cfg.ffn
    for tag, M in (("pf_", rows), ("pfl_", seqs), ("dc_", seqs)):
        if M:
            ws.get(tag + "qkv", (M, W), BF16).fill_(NAN)
            ws.get(tag + "att", (M, hd), BF16).fill_(NAN)
            ws.get(tag + "act", (M, I), BF16).fill_(NAN)
    if seqs:
        ws.get("pfl_q", (seqs, hd), BF16).fill_(NAN)
        ws.get("pfl_h", (seqs, hd), F32).fill_(NAN)
        ws.get("dc_logits_xn", (seqs, hd), BF16).fill_(NAN)
        ws.get("dc_logits", (seqs, cfg.vocab), F32).fill_(NAN)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases both test modules run (tests/test_decoder_stages.py on the emulation, tests/test_gpu_decoder_stages.py on the kernels)
# ---------------------------------------------------------------------------------------------------------------------------
PREFILL_LENS = [1, 5, 64, 65, 200]             # one row, both sides of the 64-key tile, several tiles
DECODE_LENS = (63, 1, 5, 30, 64)               # prompt lengths of the decode rows, cycled; row 0 crosses 63 -> 64 -> 65
DECODE_LONGEST = 70                            # the last row's prompt: its third step sits at max_len - 1
DECODE_STEPS = 3


def family_cfg(name):
    """The tiny decoders of the stage tests -> (LlamaCfg, state-dict prefix)."""
    from dataclasses import replace
    from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
    a = SalmonnCfg.tiny().llama
    if name == "b":
        return QwenAudioCfg.tiny().llm, "language_model."
    return {"a": a, "c": replace(a, n_heads=4), "d": replace(a, n_kv_heads=1), "e": replace(a, qk_norm=True),
            "e_gqa": replace(a, qk_norm=True, n_kv_heads=1), "f": replace(a, lora_rank=0)}[name], "llama_model."


def family_state(cfg, prefix, device, seed=0):
    from icl_speech_text_llm_amd.runtime import synth
    return synth.llama_state(cfg, synth._Gen(seed, device, torch.float32, jitter=True), prefix=prefix)


def prefill_form(rt, M, kv, last_rows_only):
    """Which of its forms a prefill over M packed rows takes, from the public predicates of runtime.binding."""
    import icl_speech_text_llm_amd.runtime.binding as B
    c = rt.w.cfg
    plain = c.group == 1 and not c.qk_norm
    return dict(epilogue=plain and B.rope_fusable(M, c.n_heads, c.head_dim, rt.w.k_aug), fp8=kv == "fp8", last_rows_only=last_rows_only,
                trim=bool(last_rows_only and rt.prefill_last_rows and kv == "bf16" and plain
                          and B.rope_epilogue_ok(c.n_heads, c.head_dim, rt.w.k_aug)))


def _tokens(cfg, lens, seed):
    from decoder_support import row_prompts
    return [p[0] for p in row_prompts(cfg.vocab, lens, seed)]


def _i32(x, dev):
    return torch.tensor(list(x), dtype=I32, device=dev)


def run_prefill(rt, ws, sd, prefix, seq_lens, *, kv=None, last_rows_only=False, max_len=None, speech_rows=0, chunk=None, seed=100,
                want_logits=True, mutate=None, ws_hook=None):
    """embed + prefill (+ logits) of ``rt`` over seeded prompts of ``seq_lens`` positions, recorded and walked -> (worst, number
    of launches, the prefill form).  ``speech_rows``: that many rows of the longest prompt come from a speech tensor;
    ``chunk``: prefill sequences [0, chunk) and [chunk, n) in two calls through ``cache.rows``; ``mutate``: a planted mistake
    (``recording``), called with the cache as a fourth argument."""
    from icl_speech_text_llm_amd.runtime import engines as E
    cfg, dev = rt.w.cfg, rt.w.embed.device
    n, M = len(seq_lens), sum(seq_lens)
    src = [t for p in _tokens(cfg, seq_lens, seed) for t in p]
    speech = None
    if speech_rows:
        b = max(range(n), key=lambda i: seq_lens[i])
        r0 = oa.cu_of(seq_lens)[b] + 2
        speech = torch.randn(speech_rows, cfg.hidden, generator=torch.Generator().manual_seed(seed)).to(dev)
        for j in range(speech_rows):
            src[r0 + j] = -1 - j
    max_len = max_len or max(seq_lens) + DECODE_STEPS
    cache = E.KVCache(cfg, n, max_len, ws, dtype=kv) if kv else None
    if cache is not None:
        poison_cache(cache)
    poison_workspace(ws, cfg, M, n)
    plant = None if mutate is None else (lambda name, k, a: mutate(name, k, a, cache))
    worst, count = {}, 0
    merge = lambda d: worst.update({k: max(worst.get(k, 0.0), v) for k, v in d.items()})
    if chunk is None:
        form = prefill_form(rt, M, kv, last_rows_only)
        with recording(plant) as launches:
            h = rt.embed(ws, _i32(src, dev), speech)
            out = rt.prefill(ws, h, seq_lens, cache, last_rows_only=last_rows_only).clone()
            lg = rt.logits(ws, out).clone() if want_logits else None
        merge(walk_prefill(launches, sd, prefix, cfg, src, speech, seq_lens, form, out, cache=cache, logits=lg))
        return worst, len(launches), form, cache
    h = rt.embed(ws, _i32(src, dev), speech)
    last = ws.get("gen_last", (n, cfg.hidden), F32)
    r0 = 0
    for b0, b1 in ((0, chunk), (chunk, n)):
        lens = seq_lens[b0:b1]
        r1 = r0 + sum(lens)
        form = prefill_form(rt, r1 - r0, kv, True)
        h_in = h[r0:r1].clone()
        with recording(plant) as launches:
            out = rt.prefill(ws, h[r0:r1], lens, cache.rows(b0, b1), last_rows_only=True, last_out=last[b0:b1]).clone()
        merge(walk_prefill(launches, sd, prefix, cfg, src[r0:r1], speech, lens, form, out, cache=cache, b0=b0, h_in=h_in))
        count += len(launches)
        r0 = r1
    return worst, count, form, cache


def decode_prompt_lens(Bn):
    return [DECODE_LENS[b % len(DECODE_LENS)] for b in range(Bn - 1)] + [DECODE_LONGEST]


def run_decode(rt, ws, sd, prefix, Bn, *, kv="bf16", steps=DECODE_STEPS, seed=200, prompt_lens=None, max_len=None, sd_walk=None, mutate=None):
    """An (unrecorded) prefill of Bn seeded prompts into a NaN-filled cache, then ``steps`` consecutive decode steps, each recorded
    and walked -> (worst, launches per step).  The last row's prompt is the longest: its last step is at max_len - 1."""
    from icl_speech_text_llm_amd.runtime import engines as E
    cfg, dev = rt.w.cfg, rt.w.embed.device
    plens = list(prompt_lens or decode_prompt_lens(Bn))
    max_len = max_len or max(plens) + steps
    cache = E.KVCache(cfg, Bn, max_len, ws, dtype=kv)
    poison_cache(cache)
    poison_workspace(ws, cfg, sum(plens), Bn)
    src = [t for p in _tokens(cfg, plens, seed) for t in p]
    rt.prefill(ws, rt.embed(ws, _i32(src, dev), None), plens, cache, last_rows_only=True)
    sid = _i32(range(Bn), dev)
    worst, counts = {}, []
    for t in range(steps):
        ids = _tokens(cfg, [1] * Bn, seed + 1000 * (t + 1))
        ids = [i[0] for i in ids]
        positions = [s + t for s in plens]
        poison_workspace(ws, cfg, 0, Bn)
        with recording(None if mutate is None else (lambda name, k, a: mutate(name, k, a, cache))) as launches:
            lg = rt.decode_step(ws, cache, _i32(ids, dev), _i32(positions, dev), _i32([p + 1 for p in positions], dev), sid).clone()
        got = walk_decode_step(launches, sd_walk or sd, prefix, cfg, ids, positions, cache, lg, fuse_rope=rt.fuse_decode_rope,
                               fuse_norms=rt.fuse_decode_norms)
        worst.update({k: max(worst.get(k, 0.0), v) for k, v in got.items()})
        counts.append(len(launches))
    assert max(positions) == max_len - 1
    return worst, counts
