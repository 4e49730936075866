"""Teacher-forced, stage-by-stage check of the audio encoder chains (LogMel, WhisperEncoderHIP, QwenAudioTowerHIP, BeatsHIP,
SpeechQFormerHIP of runtime/engines.py).  Not a test module and not a conftest: tests/test_gpu_encoder_stages.py runs it on the
kernels, tests/test_encoder_stages.py on the emulation of tests/encoder_emulation.py.

``recording()`` wraps every launching wrapper of runtime.binding the encoder engines use: it calls the real function, then keeps
the wrapper's name and a copy of every buffer the launch wrote (``out``, ``out2``, ``gate``, ``spec``, ``xt``; ``x`` and ``xg`` of
beats_posconv_pack) — the whole storage behind the argument, so that what lies around a view (the zero rows of a padded buffer,
the columns another launch owns) can be judged too.

The ``walk_*`` functions consume the recorded launches in order.  They first compare the kinds of the launches with what the
chain is expected to issue (``ChainChanged``: the chain changed, update the stage list — not a numeric failure), then judge
every element each launch wrote against the float64 specification of that stage (oracle/encoder_stages.py), which is computed
from the state dict and the logical contents of the PREVIOUS stage's actual output: errors do not accumulate, so each stage is
held to the bound its kernel family already has (tests/fp64_bounds.py, oracle/attention.py) and no tolerance is introduced here.
f32 GEMM / norm / gate / axpby outputs: the bound itself; bf16 GEMM outputs: + one bf16 ulp (bf16_out_bound); bf16 outputs of the
other kernels: the interval [bf16(ref - e), bf16(ref + e)]; attention: err_bound with the kernel's r_P; data movers, zero rows and
second outputs (out2 = bf16(out)): bit for bit.  A miss raises ``StageFailure`` naming the stage and the first element.
``Walk.worst`` holds the largest err / bound per stage kind."""
import contextlib
import functools
import inspect

import torch

import fp64_bounds as fb
from oracle import attention as oa
from oracle import encoder_stages as es
from oracle import models as om

BF16, F32 = torch.bfloat16, torch.float32

WRITTEN = dict(gemm=("out",), layernorm=("out", "out2"), attn_fwd=("out",), qformer_window_xattn=("out",), beats_gate=("gate",),
               axpby_cast=("out",), logmel_whisper=("spec", "xt"), spec_to_xt=("xt",), fbank_kaldi=("out",),
               beats_patchify=("out",), beats_posconv_pack=("x", "xg"))


class ChainChanged(AssertionError):
    pass


class StageFailure(AssertionError):
    def __init__(self, stage, msg):
        super().__init__(f"stage {stage}: {msg}")
        self.stage = stage


class Written:
    """A copy of the storage behind one written argument, and the argument's geometry in it."""

    def __init__(self, t):
        whole = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())
        self.flat, self.shape, self.stride, self.offset = whole.clone(), tuple(t.shape), tuple(t.stride()), t.storage_offset()

    def view(self):
        """What the argument showed after the launch."""
        return torch.as_strided(self.flat, self.shape, self.stride, self.offset)

    def base(self, shape):
        """The buffer the argument is a view of, from its first element, in ``shape``."""
        n = 1
        for s in shape:
            n *= s
        return self.flat[:n].view(shape)


class Launch:
    def __init__(self, name, written):
        self.name, self.written = name, written

    def __getitem__(self, arg):
        return self.written[arg]


@contextlib.contextmanager
def recording():
    """-> the list of ``Launch`` records, appended to as the encoder wrappers of runtime.binding are called."""
    import icl_speech_text_llm_amd.runtime.binding as B
    saved = {n: getattr(B, n) for n in WRITTEN}
    launches = []

    def wrapper(name, f):
        sig = inspect.signature(f)

        @functools.wraps(f)
        def call(*args, **kwargs):
            r = f(*args, **kwargs)
            bound = sig.bind(*args, **kwargs).arguments
            launches.append(Launch(name, {a: Written(bound[a]) for a in WRITTEN[name] if bound.get(a) is not None}))
            return r
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
def _first(bad):
    return bad.nonzero()[0].tolist()


class Walk:
    def __init__(self, launches, expected):
        got = [l.name for l in launches]
        if got != list(expected):
            k = next((i for i, (a, b) in enumerate(zip(got, expected)) if a != b), min(len(got), len(expected)))
            raise ChainChanged(f"the chain changed, update the stage list: {len(got)} launches against {len(expected)} expected, "
                               f"first difference at launch {k}: got {got[k:k + 3]}, expected {list(expected)[k:k + 3]}")
        self.launches, self.i, self.worst = launches, 0, {}

    def take(self, name):
        l = self.launches[self.i]
        assert l.name == name, (self.i, l.name, name)
        self.i += 1
        return l

    def done(self):
        assert self.i == len(self.launches), f"{len(self.launches) - self.i} launches left unjudged"

    def _note(self, stage, kind, ratio, bad):
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)
        if bool(bad.any()):
            raise StageFailure(stage, f"{int(bad.sum())} of {bad.numel()} elements outside the {kind} bound, first at "
                                      f"{_first(bad)}, worst err/bound {ratio:.3g}")

    def f32(self, stage, kind, got, ref, e):
        assert got.dtype == F32 and got.shape == ref.shape, (stage, got.dtype, got.shape, ref.shape)
        self._note(stage, kind, fb.worst_ratio(got, ref, e), ~fb.within(got, ref, e))

    def gemm_bf16(self, stage, got, ref, e):
        assert got.dtype == BF16 and got.shape == ref.shape, (stage, got.dtype, got.shape, ref.shape)
        e = fb.bf16_out_bound(e, ref, got)
        self._note(stage, "gemm", fb.worst_ratio(got, ref, e), ~fb.within(got, ref, e))

    def interval(self, stage, kind, got, ref, e):
        assert got.dtype == BF16 and got.shape == ref.shape, (stage, got.dtype, got.shape, ref.shape)
        got, ref, e = got.cpu(), ref.cpu(), e.cpu()             # as tests/test_gpu_glue_exact.py judges its intervals
        lo, hi = fb.bf16_interval(ref, e)
        # its own kind: an output that IS an end of its interval reads 1.000, which says nothing about the f32 outputs' margin
        self._note(stage, kind + "_bf16", fb.interval_ratio(got, ref, lo, hi), ~fb.in_interval(got, lo, hi))

    def attention(self, stage, kind, got, R, D, r_P):
        bad, worst = oa.fails_bound(got.reshape(R.ref.shape), R, D, r_P)
        self.worst[kind] = max(self.worst.get(kind, 0.0), worst)
        if bool(bad.any()):
            raise StageFailure(stage, f"err/bound {worst:.3g} > 1 at {oa.describe(R, bad)}")

    def exact(self, stage, got, want):
        assert got.dtype == want.dtype and got.shape == want.shape, (stage, got.dtype, want.dtype, got.shape, want.shape)
        self.worst.setdefault("exact", 0.0)
        if not es.same_bits(got, want):
            iv = torch.int16 if got.element_size() == 2 else torch.int32
            bad = got.contiguous().view(iv) != want.contiguous().view(iv)
            self.worst["exact"] = float("inf")
            raise StageFailure(stage, f"{int(bad.sum())} of {bad.numel()} elements differ from the exact image, first at {_first(bad)}")


def report(case, worst):
    for kind in sorted(worst):
        print(f"err/bound encoder stages {case} {kind}: {worst[kind]:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# expected launches of each chain
# ---------------------------------------------------------------------------------------------------------------------------
def whisper_kinds(n_layers, final_ln=True):
    return (["gemm", "gemm"] + ["layernorm", "gemm", "attn_fwd", "gemm", "layernorm", "gemm", "gemm"] * n_layers
            + (["layernorm"] if final_ln else []))


def qwen_kinds(n_layers):
    return whisper_kinds(n_layers, False) + ["axpby_cast", "axpby_cast", "layernorm", "gemm"]


def beats_kinds(T, n_layers, groups):
    uniform = all(t == T[0] for t in T)                      # equal clips run one batched GEMM per group, others one per clip
    return (["fbank_kaldi", "beats_patchify", "gemm", "layernorm", "gemm", "beats_posconv_pack"]
            + ["gemm"] * (groups * (1 if uniform else len(T))) + ["layernorm"]
            + ["gemm", "beats_gate", "attn_fwd", "gemm", "layernorm", "gemm", "gemm", "layernorm"] * n_layers)


def qformer_runs(n, T_audio):
    """Runs (a0, a1, T) of consecutive clips with the same frame count T = max(1500, BEATs tokens)."""
    frames = [1500 if T_audio is None else max(1500, T_audio[a]) for a in range(n)]
    runs, a0 = [], 0
    while a0 < n:
        a1 = a0 + 1
        while a1 < n and frames[a1] == frames[a0]:
            a1 += 1
        runs.append((a0, a1, frames[a0]))
        a0 = a1
    return runs


def qformer_kinds(n, T_audio, n_layers):
    out = []
    for a0, a1, T in qformer_runs(n, T_audio):
        out += ["layernorm"] * (1 if T == 1500 else a1 - a0) + (["layernorm"] * (a1 - a0) if T_audio is not None else [])
        out += ["layernorm", "axpby_cast", "axpby_cast"]
        out += ["gemm", "gemm", "layernorm", "gemm", "gemm", "qformer_window_xattn", "gemm", "layernorm", "gemm", "gemm",
                "layernorm"] * n_layers + ["gemm"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the chains
# ---------------------------------------------------------------------------------------------------------------------------
def walk_logmel(w, wav, lens, n_mels, tag="logmel"):
    """-> the mel frames the conv stem reads, [n, 3000, n_mels] bf16 (the logical contents of xt)."""
    l = w.take("logmel_whisper")
    xt = l["xt"].view()
    dev, n = xt.device, xt.shape[0]
    refs = [es.logmel(wav[b, :int(L)].cpu().numpy(), n_mels) for b, L in enumerate(lens)]
    if "spec" in l.written:
        spec = l["spec"].view()
        for b, (ref, e) in enumerate(refs):
            w.f32(f"{tag}.spec", "logmel", spec[b], ref.to(dev), e.to(dev))
        w.exact(f"{tag}.xt", xt, es.xt_of_spec(spec, xt.shape[2]))
    else:
        for b, (ref, e) in enumerate(refs):
            w.interval(f"{tag}.xt", "logmel", xt[b, 1:3001, :n_mels], ref.t().to(dev), e.t().to(dev))
        z = xt.clone()
        z[:, 1:3001, :n_mels] = 0
        w.exact(f"{tag}.xt_zero", z, torch.zeros_like(z))
    assert xt.shape[0] == n and xt.shape[1] == 3002
    return xt[:, 1:3001, :n_mels]


def walk_spec_to_xt(w, spec, tag="spec_to_xt"):
    xt = w.take("spec_to_xt")["xt"].view()
    w.exact(tag, xt, es.xt_of_spec(spec, xt.shape[2]))
    return xt[:, 1:3001, :spec.shape[1]]


def walk_whisper(w, sd, p, n_heads, mel, kv_lens=None, final_ln=True, tag="whisper"):
    """mel [n, 3000, n_mels] -> the encoder's output rows [n 1500, d] (as the chain wrote them)."""
    n, T = mel.shape[0], 1500
    x1 = w.take("gemm")["out"].view()[:, :3000]                              # conv1 writes frames 1 .. 3000 of the padded buffer
    w.gemm_bf16(f"{tag}.conv1", x1, *es.whisper_conv1(sd, p, mel))
    d = x1.shape[2]
    h = w.take("gemm")["out"].view()
    w.f32(f"{tag}.conv2", "gemm", h.view(n, T, d), *es.whisper_conv2(sd, p, x1))
    for i in range(es.n_layers_of(sd, p + "layers.")):
        lp, st = f"{p}layers.{i}.", f"{tag}.L{i}."
        xn = w.take("layernorm")["out"].view()
        w.interval(st + "ln1", "norm", xn, *es.layer_norm(sd, lp + "self_attn_layer_norm", h, 1e-5))
        qkv = w.take("gemm")["out"].view()
        w.gemm_bf16(st + "qkv", qkv, *es.linear(sd, [lp + "self_attn.q_proj", lp + "self_attn.k_proj", lp + "self_attn.v_proj"], xn))
        att = w.take("attn_fwd")["out"].view()
        R, D = es.self_attention(qkv, [T] * n, n_heads, kv_lens=kv_lens)
        w.attention(st + "attn", "attention", att, R, D, oa.R_P[f"prefill{D}"])
        h2 = w.take("gemm")["out"].view()
        w.f32(st + "out_proj", "gemm", h2, *es.linear(sd, lp + "self_attn.out_proj", att, residual=h))
        h = h2
        xn = w.take("layernorm")["out"].view()
        w.interval(st + "ln2", "norm", xn, *es.layer_norm(sd, lp + "final_layer_norm", h, 1e-5))
        ff = w.take("gemm")["out"].view()
        w.gemm_bf16(st + "fc1", ff, *es.linear(sd, lp + "fc1", xn, gelu=True))
        h2 = w.take("gemm")["out"].view()
        w.f32(st + "fc2", "gemm", h2, *es.linear(sd, lp + "fc2", ff, residual=h))
        h = h2
    if not final_ln:
        return h
    out = w.take("layernorm")["out"].view()
    w.f32(f"{tag}.ln_post", "norm", out, *es.layer_norm(sd, p + "layer_norm", h, 1e-5))
    return out


def walk_qwen(launches, sd, n_heads, spec, mel_lens, result):
    """QwenAudioRuntime.encode_audio(input_features=spec, mel_lens): spec_to_xt, the tower, the pool, ln_post, the projector."""
    p = "audio_tower."
    L = es.n_layers_of(sd, p + "layers.")
    w = Walk(launches, ["spec_to_xt"] + qwen_kinds(L))
    mel = walk_spec_to_xt(w, spec)
    n, T = mel.shape[0], 1500
    h = walk_whisper(w, sd, p, n_heads, mel, kv_lens=es.qwen_key_lens(mel_lens), final_ln=False, tag="qwen")
    d = h.shape[1]
    even, odd = es.pool_pairs(h.view(n, T, d))
    p1 = w.take("axpby_cast")["out"].view()
    w.f32("qwen.pool_odd", "axpby", p1, *fb.axpby_ref_bound(odd.reshape(-1, d), 0.5))
    p2 = w.take("axpby_cast")["out"].view()
    w.f32("qwen.pool_even", "axpby", p2, *fb.axpby_ref_bound(even.reshape(-1, d), 0.5, add=p1))
    pb = w.take("layernorm")["out"].view()
    w.interval("qwen.ln_post", "norm", pb, *es.layer_norm(sd, p + "layer_norm", p2, 1e-5))
    out = w.take("gemm")["out"].view()
    w.f32("qwen.projector", "gemm", out, *es.linear(sd, "multi_modal_projector.linear", pb))
    w.done()
    feats, lens = result
    w.exact("qwen.result", feats.reshape(out.shape), out)
    want = [om.qwen_audio_lengths(int(m))[1] for m in mel_lens]
    if list(lens) != want:
        raise StageFailure("qwen.lengths", f"valid rows {list(lens)} against {want}")
    return w.worst


def walk_beats(w, sd, p, cfg, wav, padded_lens, valid_lens, tag="beats"):
    """-> (x [sum T, d] as the chain left it, cu, T)."""
    n = len(padded_lens)
    shapes = [es.beats_shape(pl, vl) for pl, vl in zip(padded_lens, valid_lens)]
    nf, T, pm = [s[0] for s in shapes], [s[1] for s in shapes], [s[2] for s in shapes]
    cu = oa.cu_of(T)
    M, G = cu[-1], cfg.conv_groups
    fbk = w.take("fbank_kaldi")["out"].view()
    dev = fbk.device
    pm = [m.to(dev) for m in pm]
    for a in range(n):
        ref, e = es.fbank(wav[a, :int(padded_lens[a])].cpu().numpy(), cfg.fbank_mean, cfg.fbank_std)
        w.f32(f"{tag}.fbank", "fbank", fbk[a, :nf[a]], ref.to(dev), e.to(dev))
    patches = w.take("beats_patchify")["out"].view()
    w.exact(f"{tag}.patchify", patches, torch.cat([es.patches_of(fbk[a], T[a]) for a in range(n)]))
    e0 = w.take("gemm")["out"].view()
    w.f32(f"{tag}.patch_embed", "gemm", e0, *es.patch_embed(sd, p, patches))
    eb = w.take("layernorm")["out"].view()
    w.interval(f"{tag}.ln0", "norm", eb, *es.layer_norm(sd, p + "layer_norm", e0, 1e-5))
    x = w.take("gemm")["out"].view()
    w.f32(f"{tag}.post_extract_proj", "gemm", x, *es.linear(sd, p + "post_extract_proj", eb))
    d = x.shape[1]
    cpg = d // G
    l = w.take("beats_posconv_pack")
    xm, want = l["x"].view(), x.clone()
    for a in range(n):
        want[cu[a]:cu[a + 1]][pm[a]] = 0
    w.exact(f"{tag}.posconv_pack.x", xm, want)
    img = []
    for a in range(n):
        g = torch.zeros(G, T[a] + 128, cpg, dtype=BF16, device=dev)
        g[:, 64:64 + T[a]] = xm[cu[a]:cu[a + 1]].to(BF16).view(T[a], G, cpg).transpose(0, 1)
        img.append(g.reshape(-1))
    w.exact(f"{tag}.posconv_pack.xg", l["xg"].view(), torch.cat(img))
    for _ in range(G * (1 if all(t == T[0] for t in T) else n)):
        last = w.take("gemm")
    y = last["out"].base((M, d))                                              # the finished y: every group of every clip
    for a in range(n):
        w.f32(f"{tag}.posconv", "gemm", y[cu[a]:cu[a + 1]], *es.posconv(sd, p, xm[cu[a]:cu[a + 1]], G))
    l = w.take("layernorm")
    x, xb = l["out"].view(), l["out2"].view()
    w.f32(f"{tag}.encoder_ln", "norm", x, *es.layer_norm(sd, p + "encoder.layer_norm", y, 1e-5))
    w.exact(f"{tag}.encoder_ln.out2", xb, x.to(BF16))
    n_layers = es.n_layers_of(sd, p + "encoder.layers.")
    alpha = (2.0 * n_layers) ** 0.25                                           # deep_norm_alpha, as beats_encoder has it
    assert alpha == cfg.deep_norm_alpha
    table = es.rel_table(sd, p, max(T), cfg).to(dev)
    kvl = [int((~m).sum()) for m in pm]
    for i in range(n_layers):
        lp, st = f"{p}encoder.layers.{i}.", f"{tag}.L{i}."
        qkv = w.take("gemm")["out"].view()
        w.gemm_bf16(st + "qkv", qkv, *es.linear(sd, [lp + "self_attn.q_proj", lp + "self_attn.k_proj", lp + "self_attn.v_proj"], xb))
        gate = w.take("beats_gate")["gate"].view()
        w.f32(st + "gate", "gate", gate, *es.beats_gate(sd, lp, qkv[:, :d], cfg.n_heads))
        att = w.take("attn_fwd")["out"].view()
        R, D = es.self_attention(qkv, T, cfg.n_heads, kv_lens=kvl, rel_bias=table, rel_gate=gate)
        w.attention(st + "attn", "attention", att, R, D, oa.R_P[f"prefill{D}"])
        o = w.take("gemm")["out"].view()
        w.f32(st + "out_proj", "gemm", o, *es.linear(sd, lp + "self_attn.out_proj", att))
        x, xb = _deep_norm(w, sd, lp + "self_attn_layer_norm", st + "ln1", o, x, alpha)
        ff = w.take("gemm")["out"].view()
        w.gemm_bf16(st + "fc1", ff, *es.linear(sd, lp + "fc1", xb, gelu=True))
        o = w.take("gemm")["out"].view()
        w.f32(st + "fc2", "gemm", o, *es.linear(sd, lp + "fc2", ff))
        x, xb = _deep_norm(w, sd, lp + "final_layer_norm", st + "ln2", o, x, alpha)
    return x, cu, T


def _deep_norm(w, sd, name, stage, o, x, alpha):
    """BEATs' post-LN step LN(alpha x + o), written over x with its bf16 copy -> (x, xb) as the launch left them."""
    l = w.take("layernorm")
    x2, xb = l["out"].view(), l["out2"].view()
    w.f32(stage, "norm", x2, *es.layer_norm(sd, name, o, 1e-5, res=x, alpha=alpha))
    w.exact(stage + ".out2", xb, x2.to(BF16))
    return x2, xb


def walk_qformer(w, sd, cfg, n_heads, speech, audio, cu, T_audio, tag="qformer"):
    """speech [n 1500, dw] f32, audio [sum T_a, db] f32 or None -> (per clip: its windows' projected rows [n_win, H_llm])."""
    n, dw, dev = speech.shape[0] // 1500, speech.shape[1], speech.device
    db = 0 if audio is None else audio.shape[1]
    hq = sd["speech_query_tokens"].shape[-1]
    n_layers = es.n_layers_of(sd, es.QF + "encoder.layer.")
    outs = []
    for a0, a1, T in qformer_runs(n, T_audio):
        nr = a1 - a0
        win, stride, nw = es.window_shape(T, cfg.second_per_window, cfg.second_stride)
        assert win == stride
        want = torch.zeros(nr * T, dw + db, dtype=BF16, device=dev)
        # K6: ln_speech | ln_audio side by side; the shorter stream is padded with zero frames AFTER its LayerNorm
        if T == 1500:
            l = w.take("layernorm")
            got = l["out"].view()[:, :dw]
            w.interval(f"{tag}.ln_speech", "norm", got, *es.layer_norm(sd, "ln_speech", speech[a0 * 1500:a1 * 1500], 1e-5))
            want[:, :dw] = got
        else:
            for a in range(a0, a1):
                l = w.take("layernorm")
                got = l["out"].view()[:, :dw]
                w.interval(f"{tag}.ln_speech", "norm", got, *es.layer_norm(sd, "ln_speech", speech[a * 1500:(a + 1) * 1500], 1e-5))
                want[(a - a0) * T:(a - a0) * T + 1500, :dw] = got
        if audio is not None:
            for a in range(a0, a1):
                l = w.take("layernorm")
                got = l["out"].view()
                w.interval(f"{tag}.ln_audio", "norm", got, *es.layer_norm(sd, "ln_audio", audio[cu[a]:cu[a + 1]], 1e-5))
                want[(a - a0) * T:(a - a0) * T + T_audio[a], dw:] = got
        cat = l["out"].base((nr * T, dw + db))
        w.exact(f"{tag}.cat", cat, want)                                      # each block where it belongs, zeros everywhere else
        q0 = w.take("layernorm")["out"].view()
        query = es._p(sd, "speech_query_tokens", dev).reshape(1, hq)
        w.f32(f"{tag}.query_ln", "norm", q0, *es.layer_norm(sd, es.QF + "embeddings.LayerNorm", query, cfg.ln_eps))
        W = nr * nw
        h = w.take("axpby_cast")["out"].view()
        w.f32(f"{tag}.broadcast_f32", "axpby", h, *fb.axpby_ref_bound(q0.expand(W, hq), 1.0))
        hb = w.take("axpby_cast")["out"].view()
        w.interval(f"{tag}.broadcast_bf16", "axpby", hb, *fb.axpby_ref_bound(q0.expand(W, hq), 1.0))
        for i in range(n_layers):
            lp, st = f"{es.QF}encoder.layer.{i}.", f"{tag}.L{i}."
            # self-attention over the window's one query token: the softmax is 1, the context is the value projection
            tb = w.take("gemm")["out"].view()
            w.gemm_bf16(st + "sa_value", tb, *es.linear(sd, lp + "attention.self.value", hb))
            t32 = w.take("gemm")["out"].view()
            w.f32(st + "sa_out", "gemm", t32, *es.linear(sd, lp + "attention.output.dense", tb, residual=h))
            l = w.take("layernorm")
            h, hb = l["out"].view(), l["out2"].view()
            w.f32(st + "sa_ln", "norm", h, *es.layer_norm(sd, lp + "attention.output.LayerNorm", t32, cfg.ln_eps))
            w.exact(st + "sa_ln.out2", hb, h.to(BF16))
            q = w.take("gemm")["out"].view()
            w.gemm_bf16(st + "ca_query", q, *es.linear(sd, lp + "crossattention.self.query", hb))
            kv = w.take("gemm")["out"].view()
            w.gemm_bf16(st + "ca_kv", kv, *es.linear(sd, [lp + "crossattention.self.key", lp + "crossattention.self.value"], cat))
            tb = w.take("qformer_window_xattn")["out"].view()
            w.attention(st + "xattn", "qformer_attention", tb, es.window_attention(q, kv, nr, T, win, nw, n_heads), 64,
                        oa.R_P["qformer"])
            t32 = w.take("gemm")["out"].view()
            w.f32(st + "ca_out", "gemm", t32, *es.linear(sd, lp + "crossattention.output.dense", tb, residual=h))
            l = w.take("layernorm")
            h, hb = l["out"].view(), l["out2"].view()
            w.f32(st + "ca_ln", "norm", h, *es.layer_norm(sd, lp + "crossattention.output.LayerNorm", t32, cfg.ln_eps))
            w.exact(st + "ca_ln.out2", hb, h.to(BF16))
            ff = w.take("gemm")["out"].view()
            w.gemm_bf16(st + "ffn1", ff, *es.linear(sd, lp + "intermediate_query.dense", hb, gelu=True))
            t32 = w.take("gemm")["out"].view()
            w.f32(st + "ffn2", "gemm", t32, *es.linear(sd, lp + "output_query.dense", ff, residual=h))
            l = w.take("layernorm")
            h, hb = l["out"].view(), l["out2"].view()
            w.f32(st + "ffn_ln", "norm", h, *es.layer_norm(sd, lp + "output_query.LayerNorm", t32, cfg.ln_eps))
            w.exact(st + "ffn_ln.out2", hb, h.to(BF16))
        out = w.take("gemm")["out"].view()
        w.f32(f"{tag}.projector", "gemm", out, *es.linear(sd, "speech_llama_proj", hb))
        outs += list(out.view(nr, nw, -1))
    return outs


def walk_salmonn(launches, sd, cfg, wav, wav_lens, padded_lens, result):
    """One SalmonnRuntime.encode_speech(wav, wav_lens, padded_lens=...) call: log-mel, Whisper, BEATs, Q-Former, and the
    placement of each clip's windows in the returned [n, W_max, H_llm] (zeros past the clip's own window count)."""
    n = len(wav_lens)
    padded = list(wav_lens if padded_lens is None else padded_lens)
    use_beats = cfg.beats is not None
    T_audio = [es.beats_shape(pl, vl)[1] for pl, vl in zip(padded, wav_lens)] if use_beats else None
    wl = es.n_layers_of(sd, "speech_encoder.layers.")
    kinds = ["logmel_whisper"] + whisper_kinds(wl)
    if use_beats:
        kinds += beats_kinds(T_audio, es.n_layers_of(sd, "beats.encoder.layers."), cfg.beats.conv_groups)
    kinds += qformer_kinds(n, T_audio, es.n_layers_of(sd, es.QF + "encoder.layer."))
    w = Walk(launches, kinds)
    mel = walk_logmel(w, wav, wav_lens, cfg.whisper.n_mels)
    speech = walk_whisper(w, sd, "speech_encoder.", cfg.whisper.n_heads, mel)
    audio = cu = None
    if use_beats:
        audio, cu, T_audio = walk_beats(w, sd, "beats.", cfg.beats, wav, padded, wav_lens)
    outs = walk_qformer(w, sd, cfg.qformer, cfg.qformer.n_heads, speech, audio, cu, T_audio)
    w.done()
    Wmax = max(o.shape[0] for o in outs)
    want = torch.zeros(n, Wmax, outs[0].shape[1], dtype=F32, device=outs[0].device)
    for a, o in enumerate(outs):
        want[a, :o.shape[0]] = o
    w.exact("qformer.result", result.reshape(want.shape), want)
    return w.worst


# ---------------------------------------------------------------------------------------------------------------------------
# one engine at a time (the planted mistakes of tests/test_encoder_stages.py run the engine they are planted in)
# ---------------------------------------------------------------------------------------------------------------------------
def check_whisper(launches, sd, cfg, xt):
    """WhisperEncoderHIP.forward(ws, xt) on its own; xt [n, 3002, 128] as given to it."""
    w = Walk(launches, whisper_kinds(es.n_layers_of(sd, "speech_encoder.layers.")))
    walk_whisper(w, sd, "speech_encoder.", cfg.whisper.n_heads, xt[:, 1:3001, :cfg.whisper.n_mels])
    w.done()
    return w.worst


def check_beats(launches, sd, cfg, wav, padded_lens, valid_lens, result):
    T = [es.beats_shape(pl, vl)[1] for pl, vl in zip(padded_lens, valid_lens)]
    w = Walk(launches, beats_kinds(T, es.n_layers_of(sd, "beats.encoder.layers."), cfg.beats.conv_groups))
    x, cu, T = walk_beats(w, sd, "beats.", cfg.beats, wav, padded_lens, valid_lens)
    w.done()
    w.exact("beats.result", result[0], x)
    if list(result[1]) != cu or list(result[2]) != T:
        raise StageFailure("beats.result", f"row offsets / token counts {result[1]} {result[2]} against {cu} {T}")
    return w.worst


def check_qformer(launches, sd, cfg, speech, audio, cu, result):
    n = speech.shape[0] // 1500
    T_audio = None if audio is None else [cu[a + 1] - cu[a] for a in range(n)]
    w = Walk(launches, qformer_kinds(n, T_audio, es.n_layers_of(sd, es.QF + "encoder.layer.")))
    outs = walk_qformer(w, sd, cfg.qformer, cfg.qformer.n_heads, speech, audio, cu, T_audio)
    w.done()
    Wmax = max(o.shape[0] for o in outs)
    want = torch.zeros(n, Wmax, outs[0].shape[1], dtype=F32, device=outs[0].device)
    for a, o in enumerate(outs):
        want[a, :o.shape[0]] = o
    w.exact("qformer.result", result.reshape(want.shape), want)
    return w.worst


# ---------------------------------------------------------------------------------------------------------------------------
# the runtimes' encoder halves on CPU tensors (for the emulation: the constructors themselves insist on a GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def cpu_salmonn(cfg, sd):
    from icl_speech_text_llm_amd.runtime import engines as E, packing as P
    from icl_speech_text_llm_amd.runtime.salmonn import SalmonnRuntime
    rt = object.__new__(SalmonnRuntime)
    rt.cfg, rt.device, rt.ws = cfg, torch.device("cpu"), E.Workspace("cpu")
    rt.logmel = E.LogMel(cfg.whisper.n_mels, "cpu")
    rt.whisper = E.WhisperEncoderHIP(P.pack_whisper(sd, cfg.whisper, "cpu"))
    rt.beats = E.BeatsHIP(P.pack_beats(sd, cfg.beats, "cpu"), "cpu") if cfg.beats is not None else None
    rt.qformer = E.SpeechQFormerHIP(P.pack_qformer(sd, cfg.qformer, "cpu"), cfg.whisper.d_model,
                                    cfg.beats.d_model if cfg.beats is not None else 0, cfg.llama.hidden)
    return rt


def cpu_qwen(cfg, sd):
    from icl_speech_text_llm_amd.runtime import engines as E, packing as P
    from icl_speech_text_llm_amd.runtime.qwen import QwenAudioRuntime
    rt = object.__new__(QwenAudioRuntime)
    rt.cfg, rt.device, rt.ws = cfg, torch.device("cpu"), E.Workspace("cpu")
    rt.logmel = E.LogMel(cfg.audio.n_mels, "cpu")
    enc = E.WhisperEncoderHIP(P.pack_whisper(sd, cfg.audio, "cpu", prefix="audio_tower."))
    rt.tower = E.QwenAudioTowerHIP(enc, P._bf(sd["multi_modal_projector.linear.weight"], "cpu"),
                                   P._f32(sd["multi_modal_projector.linear.bias"], "cpu"), cfg.llm.hidden)
    return rt


def check_packed(sd, rt):
    """The packed weights the stages depend on, bit for bit against the state dict re-laid-out from the definition."""
    if getattr(rt, "tower", None) is not None:
        es.check_packed_whisper(sd, rt.tower.enc.w, "audio_tower.")
        return
    es.check_packed_whisper(sd, rt.whisper.w, "speech_encoder.")
    if rt.beats is not None:
        es.check_packed_beats(sd, rt.beats.w, "beats.")
