"""Kernel chains of the ICL hot path: each engine strings libicl_hip entry points together over
buffers that stay resident in HBM (allocated once per shape through ``Workspace``; PyTorch is used
for memory and streams only — every arithmetic step below is a C-ABI call).

Stages:  K1 log-mel -> K2/K3 Whisper encoder ‖ K4/K5 BEATs -> K6 LN+concat ->
K7 window Q-Former -> K8 projector -> K9 embedding interleave -> K10 Llama prefill -> K11 decode.
Reference call sites: models/custom_salmon.py:546-554 (encode_speech), :115-299 (prompt wrap),
:556-640 (forward), :642-739 (generate_output).
"""
from __future__ import annotations

import os
from dataclasses import dataclass

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import binding as B
from .packing import PackedBeats, PackedLlama, PackedQFormer, PackedWhisper, qkv_offsets, qkv_width

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


class Workspace:
    """Named device buffers with a CAPACITY: one flat allocation per (name, dtype) that only ever grows to the largest
    request seen, handed out as a leading ``[:numel]`` view in the requested shape.  Ragged batches (a new total row count
    on almost every call) therefore reuse the same storage — resident bytes are bounded by the largest batch, not by
    the number of distinct shapes — and the steady-state loop performs no allocation.

    ``generation`` counts reallocations of the buffers a captured decode graph points into (``GRAPH_VISIBLE`` name prefixes):
    anything that baked raw pointers must be dropped when they move (``CausalLMRuntimeMixin`` does).  ``zero=True`` buffers carry regions the kernels never write and rely on being
    zero (conv padding rows, the LoRA augmentation tail): those regions sit at fixed flat offsets for fixed inner
    dimensions, so the buffer is zero-filled when it is (re)allocated and again whenever the inner dimensions change."""

    GRAPH_VISIBLE = ("dc_", "gen_", "kv_")      # buffers a captured decode graph bakes pointers into (decode_step, generate, cache)

    def __init__(self, device):
        self.device = torch.device(device)
        self._bufs: Dict[tuple, list] = {}      # (name, dtype) -> [flat tensor, inner dims of the last zero=True request]
        self.generation = 0

    def get(self, name: str, shape: Sequence[int], dtype, zero: bool = False) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        key = (name, dtype)
        ent = self._bufs.get(key)
        if ent is None or ent[0].numel() < n:
            # 1/16 of headroom on every allocation: ragged batches break their own size record by a fraction of a percent at a
            # time (128 prompts of 373-376 positions), and every reallocation drops the captured decode graphs — without it a
            # fresh runtime spends its first batches on eager, regrow + eager, capture
            cap = max(n, 1) + (max(n, 1) >> 4)
            if ent is not None:
                ent[0] = None                   # release the old block before asking for the larger one
                if name.startswith(self.GRAPH_VISIBLE):
                    self.generation += 1        # only a move of something a graph points into retires the graphs: an encoder
                                                # or prefill buffer growing (a longer clip, a longer prompt) leaves them valid
            flat = (torch.zeros if zero else torch.empty)(cap, dtype=dtype, device=self.device)
            ent = self._bufs[key] = [flat, shape[1:]]
        elif zero and ent[1] != shape[1:]:
            ent[0].zero_()
            ent[1] = shape[1:]
        return ent[0][:n].view(shape)

    def nbytes(self) -> int:
        return sum(e[0].numel() * e[0].element_size() for e in self._bufs.values())

    def release(self, *names: str) -> None:
        """Drop the named buffers (re-created on demand).  A graph-visible name counts as a move."""
        for key in [k for k in self._bufs if k[0] in names]:
            del self._bufs[key]
            if key[0].startswith(self.GRAPH_VISIBLE):
                self.generation += 1

    def clear(self) -> None:
        """Drop every buffer (they are re-created on demand).  Counts as a move: captured graphs are retired."""
        self._bufs.clear()
        self.generation += 1


def _i32(x, device) -> torch.Tensor:
    return torch.as_tensor(x, dtype=I32).to(device, non_blocking=True)


# ================================================================================================
# K1: log-mel + conv-stem operand
# ================================================================================================
class LogMel:
    def __init__(self, n_mels: int, device):
        # Slaney filter bank, f64 [n_mels, 201] (restated in runtime/audio_tables.py; data, not arithmetic)
        from .audio_tables import slaney_mel_filters
        self.n_mels = n_mels
        self.device = torch.device(device)
        self.filters = torch.from_numpy(slaney_mel_filters(n_mels)).to(self.device)

    def __call__(self, ws: Workspace, wav: torch.Tensor, wav_lens: torch.Tensor, want_spec: bool = False):
        """wav f32 [n, L] (device), wav_lens int32 [n] -> (xt bf16 [n, 3002, 128], spec f32 [n, n_mels, 3000] | None)"""
        n = wav.shape[0]
        xt = ws.get("logmel_xt", (n, 3002, 128), BF16)
        spec = ws.get("logmel_spec", (n, self.n_mels, 3000), F32) if want_spec else None
        scratch = ws.get("logmel_ws", (n * self.n_mels * 3000 + n,), F32)
        B.logmel_whisper(wav, wav_lens, self.filters, self.n_mels, spec, xt, scratch)
        return xt, spec

    def from_spectrogram(self, ws: Workspace, spec: torch.Tensor) -> torch.Tensor:
        n = spec.shape[0]
        xt = ws.get("logmel_xt", (n, 3002, 128), BF16)
        B.spec_to_xt(spec.contiguous(), xt)
        return xt


# ================================================================================================
# K2 + K3: Whisper encoder
# ================================================================================================
class WhisperEncoderHIP:
    def __init__(self, w: PackedWhisper):
        self.w = w

    def forward(self, ws: Workspace, xt: torch.Tensor, kv_lens: Optional[torch.Tensor] = None,
                final_ln: bool = True) -> torch.Tensor:
        """xt bf16 [n, 3002, 128] -> final-LayerNorm output f32 [n*1500, d] (or the pre-LN stream if not final_ln).
        kv_lens (device int32 [n]): key padding length per audio (Qwen2-Audio masks encoder frames past the audio)."""
        w, c = self.w, self.w.cfg
        n, d, T = xt.shape[0], c.d_model, c.n_ctx
        M = n * T
        x2 = ws.get("wh_x2", (n, 3002, d), BF16, zero=True)      # conv1 output, rows 0 / 3001 stay zero
        h = ws.get("wh_h", (M, d), F32)
        xn = ws.get("wh_xn", (M, d), BF16)
        qkv = ws.get("wh_qkv", (M, 3 * d), BF16)
        att = ws.get("wh_att", (M, d), BF16)
        ff = ws.get("wh_ff", (M, c.ffn), BF16)
        out = ws.get("wh_out", (M, d), F32)
        cu = ws.get("wh_cu", (n + 1,), I32)
        cu.copy_(torch.arange(0, M + 1, T, dtype=I32), non_blocking=True)
        # conv1 (k=3,p=1) as GEMM over the time-major padded mel: row t = xt[t:t+3, :128] (K = 384)
        B.gemm(xt, w.conv1_w, x2[:, 1:], bias=w.conv1_b, gelu=True, M=3000, K=384, lda=128, batch=n,
               stride_a=3002 * 128, stride_c=3002 * d)
        # conv2 (k=3,s=2,p=1): row t = x2[2t:2t+3, :] (lda = 2d, K = 3d), + GELU, + positional embedding
        B.gemm(x2, w.conv2_w, h, bias=w.conv2_b, gelu=True, residual=w.pos, M=T, K=3 * d, lda=2 * d, batch=n,
               stride_a=3002 * d, stride_c=T * d, stride_r=0)
        D = d // c.n_heads
        for L in w.layers:
            B.layernorm(h, L.ln1_g, L.ln1_b, xn, 1e-5)
            B.gemm(xn, L.wqkv, qkv, bias=L.bqkv)
            B.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], att, cu, T, c.n_heads, D, D ** -0.5, kv_lens=kv_lens)
            B.gemm(att, L.wo, h, bias=L.bo, residual=h)
            B.layernorm(h, L.ln2_g, L.ln2_b, xn, 1e-5)
            B.gemm(xn, L.w1, ff, bias=L.b1, gelu=True)
            B.gemm(ff, L.w2, h, bias=L.b2, residual=h)
        if not final_ln:
            return h
        B.layernorm(h, w.lnf_g, w.lnf_b, out, 1e-5)
        return out


# ================================================================================================
# K13: Qwen2-Audio tower = Whisper-style encoder (128 mel, key padding) -> AvgPool1d(2,2) -> ln_post -> projector
# ================================================================================================
class QwenAudioTowerHIP:
    """HF Qwen2AudioEncoder + Qwen2AudioMultiModalProjector (modeling_qwen2_audio.py:289-421), reached from the
    reference at models/custom_qwen.py:188-195 / :228-234."""

    def __init__(self, enc: WhisperEncoderHIP, proj_w: torch.Tensor, proj_b: torch.Tensor, llm_hidden: int):
        self.enc, self.proj_w, self.proj_b, self.llm_hidden = enc, proj_w, proj_b, llm_hidden

    @staticmethod
    def output_lengths(mel_len: int):
        feat = (mel_len - 1) // 2 + 1          # after the stride-2 conv
        return feat, (feat - 2) // 2 + 1       # after AvgPool1d(2, 2)

    def forward(self, ws: Workspace, xt: torch.Tensor, mel_lens: List[int]) -> Tuple[torch.Tensor, List[int]]:
        """xt bf16 [n, 3002, 128], mel_lens (valid mel frames per audio) -> (features f32 [n*750, H_llm], valid rows per audio)."""
        w, c = self.enc.w, self.enc.w.cfg
        n, d, T = xt.shape[0], c.d_model, c.n_ctx
        lens = [self.output_lengths(int(m)) for m in mel_lens]
        kv = _i32([max(1, f) for f, _ in lens], xt.device)
        h = self.enc.forward(ws, xt, kv_lens=kv, final_ln=False)                 # [n*1500, d] f32
        P = n * (T // 2)
        pooled = ws.get("qa_pool", (P, d), F32)
        even, odd = h.view(P, 2 * d)[:, :d], h.view(P, 2 * d)[:, d:]           # frames 2t / 2t+1 as strided row views
        B.axpby_cast(odd, pooled, alpha=0.5)
        B.axpby_cast(even, pooled, alpha=0.5, add=pooled)
        pb = ws.get("qa_pool_bf", (P, d), BF16)
        B.layernorm(pooled, w.lnf_g, w.lnf_b, pb, 1e-5)
        out = ws.get("qa_out", (P, self.llm_hidden), F32)
        B.gemm(pb, self.proj_w, out, bias=self.proj_b)
        return out, [o for _, o in lens]


# ================================================================================================
# K4 + K5: BEATs
# ================================================================================================
class BeatsHIP:
    def __init__(self, w: PackedBeats, device):
        from .audio_tables import kaldi_mel_banks
        self.w = w
        self.banks = torch.from_numpy(kaldi_mel_banks()).to(device)

    @staticmethod
    def frames(n_samples: int) -> int:
        return 0 if n_samples < 400 else 1 + (n_samples - 400) // 160

    @classmethod
    def tokens(cls, n_samples: int) -> int:
        return (cls.frames(n_samples) // 16) * 8

    def forward(self, ws: Workspace, wav: torch.Tensor, padded_lens: List[int], valid_lens: List[int]):
        """wav f32 [n, L] zero padded.  Audio a is processed over padded_lens[a] samples (what the reference's
        BEATs sees: the collated, padded waveform) with keys/rows beyond valid_lens[a] masked.
        Returns (x f32 [sum T_a, d] packed, cu (host list), T list)."""
        w, c = self.w, self.w.cfg
        dev = wav.device
        n, d = wav.shape[0], c.d_model
        nf = [self.frames(L) for L in padded_lens]
        T = [(f // 16) * 8 for f in nf]
        assert min(T) > 0, "audio shorter than one BEATs patch (16 frames)"
        # relative positions beyond the packed span are clamped by the kernel: exact once the span covers max_distance, where
        # the bucket function has saturated (BEATs: 800 < 1504), so clips longer than 30 s need no larger table
        assert max(T) <= w.rel_span or w.rel_span > c.max_distance, "audio longer than the packed relative-position span"
        cu_h = [0]
        for t in T:
            cu_h.append(cu_h[-1] + t)
        M = cu_h[-1]
        # valid token count per audio: BEATs.forward_padding_mask applied twice (frames, then patches)
        valid_T = []
        for a in range(n):
            vf = self._valid_units(valid_lens[a], padded_lens[a], nf[a])
            valid_T.append(max(1, self._valid_units(vf, nf[a], T[a])))
        max_frames = max(nf)
        fb = ws.get("be_fbank", (n, max_frames, 128), F32)
        B.fbank_kaldi(wav, _i32(padded_lens, dev), self.banks, max_frames, c.fbank_mean, c.fbank_std, fb)
        cu = _i32(cu_h, dev)
        valid = _i32(valid_T, dev)
        patches = ws.get("be_patches", (M, 256), BF16)
        B.beats_patchify(fb, cu, M, patches)
        e = ws.get("be_e", (M, c.embed), F32)
        eb = ws.get("be_eb", (M, c.embed), BF16)
        B.gemm(patches, w.patch_w, e)
        B.layernorm(e, w.ln0_g, w.ln0_b, eb, 1e-5)
        x = ws.get("be_x", (M, d), F32)
        B.gemm(eb, w.proj_w, x, bias=w.proj_b)
        # positional grouped conv as 16 GEMMs per audio over the padded per-group image
        G, cpg = c.conv_groups, d // c.conv_groups
        xg = ws.get("be_xg", ((M + 128 * n) * d,), BF16)
        B.beats_posconv_pack(x, cu, valid, n, M, G, xg)
        y = ws.get("be_y", (M, d), F32)
        uniform = all(t == T[0] for t in T)
        for g in range(G):
            wg, bg = w.posconv_w[g], w.posconv_b[g * cpg:(g + 1) * cpg]
            if uniform:
                a_view = xg[g * (T[0] + 128) * cpg:]
                B.gemm(a_view, wg, y[:, g * cpg:], bias=bg, gelu=True, residual=x[:, g * cpg:], M=T[0], K=128 * cpg,
                       lda=cpg, batch=n, stride_a=(T[0] + 128) * d, stride_c=T[0] * d, stride_r=T[0] * d)
            else:
                for a in range(n):
                    base = (cu_h[a] + 128 * a) * d + g * (T[a] + 128) * cpg
                    B.gemm(xg[base:], wg, y[cu_h[a]:cu_h[a + 1], g * cpg:], bias=bg, gelu=True,
                           residual=x[cu_h[a]:cu_h[a + 1], g * cpg:], M=T[a], K=128 * cpg, lda=cpg)
        xb = ws.get("be_xb", (M, d), BF16)
        B.layernorm(y, w.enc_ln_g, w.enc_ln_b, x, 1e-5, out2=xb)
        qkv = ws.get("be_qkv", (M, 3 * d), BF16)
        att = ws.get("be_att", (M, d), BF16)
        o = ws.get("be_o", (M, d), F32)
        ff = ws.get("be_ff", (M, c.ffn), BF16)
        gate = ws.get("be_gate", (M, c.n_heads), F32)
        alpha = c.deep_norm_alpha
        for L in w.layers:
            B.gemm(xb, L.wqkv, qkv, bias=L.bqkv)
            B.beats_gate(qkv, L.extra["grep_w"], L.extra["grep_b"], L.extra["grep_a"], gate, c.n_heads)
            B.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], att, cu, max(T), c.n_heads, 64, 0.125,
                       kv_lens=valid, rel_bias=w.rel_table, rel_gate=gate, rel_span=w.rel_span)
            B.gemm(att, L.wo, o, bias=L.bo)
            B.layernorm(o, L.ln1_g, L.ln1_b, x, 1e-5, res=x, alpha=alpha, out2=xb)   # LN(alpha*x + attn)
            B.gemm(xb, L.w1, ff, bias=L.b1, gelu=True)
            B.gemm(ff, L.w2, o, bias=L.b2)
            B.layernorm(o, L.ln2_g, L.ln2_b, x, 1e-5, res=x, alpha=alpha, out2=xb)
        return x, cu_h, T

    @staticmethod
    def _valid_units(valid_in: int, total_in: int, n_units: int) -> int:
        """Number of leading units NOT fully padded under BEATs.forward_padding_mask: the mask over `total_in`
        inputs is trimmed to a multiple of n_units and a unit is padding iff ALL its inputs are padding."""
        if n_units == 0:
            return 0
        per = total_in // n_units
        if per == 0:
            return n_units
        return min(n_units, -(-valid_in // per)) if valid_in > 0 else 0


# ================================================================================================
# K6 + K7 + K8: LN + concat, window-level Q-Former, projector
# ================================================================================================
class SpeechQFormerHIP:
    def __init__(self, w: PackedQFormer, whisper_d: int, beats_d: int, llm_hidden: int):
        self.w, self.whisper_d, self.beats_d, self.llm_hidden = w, whisper_d, beats_d, llm_hidden
        c = w.cfg
        self.win = round(1500 * c.second_per_window / 30.0)
        self.stride = round(1500 * c.second_stride / 30.0)
        assert self.win == self.stride, "HIP path implements non-overlapping windows (kernel == stride, SURVEY.md A8)"

    def n_windows(self, T: int = 1500) -> int:
        return (T - self.win) // self.stride + 1

    def forward(self, ws: Workspace, speech: torch.Tensor, n: int, audio: Optional[torch.Tensor] = None,
                audio_cu: Optional[List[int]] = None) -> torch.Tensor:
        """speech f32 [n*1500, dw] (Whisper out), audio f32 [sum T_a, db] packed (BEATs out) -> f32 [n*W, H_llm], W = the largest
        window count of the batch (``last_windows[a]`` rows of audio a are its tokens, the rest zero).  SALMONN pads the SHORTER
        stream with zero frames (external package, `_encode_auditory_feature`; call site models/custom_salmon.py:420-430): a
        clip of up to 30 s has 1500 frames -> 88 windows; a longer one keeps its T_a > 1500 BEATs frames next to Whisper's
        1500 (the feature extractor truncates) + zeros -> (T_a - 17) // 17 + 1 windows."""
        T0 = 1500
        frames = [T0] * n if audio is None else [max(T0, audio_cu[a + 1] - audio_cu[a]) for a in range(n)]
        self.last_windows = [self.n_windows(f) for f in frames]
        if all(f == T0 for f in frames):
            return self._run(ws, speech, n, audio, audio_cu, T0)
        Wmax = max(self.last_windows)
        full = ws.get("qf_out_ragged", (n, Wmax, self.llm_hidden), F32)
        full.zero_()
        a0 = 0
        while a0 < n:                                  # runs of consecutive audios with the same frame count
            a1 = a0 + 1
            while a1 < n and frames[a1] == frames[a0]:
                a1 += 1
            cu = [x - audio_cu[a0] for x in audio_cu[a0:a1 + 1]]
            out = self._run(ws, speech[a0 * T0:a1 * T0], a1 - a0, audio[audio_cu[a0]:audio_cu[a1]], cu, frames[a0])
            nw = self.n_windows(frames[a0])
            full[a0:a1, :nw].copy_(out.view(a1 - a0, nw, self.llm_hidden))
            a0 = a1
        return full.view(n * Wmax, self.llm_hidden)

    def _run(self, ws: Workspace, speech: torch.Tensor, n: int, audio: Optional[torch.Tensor], audio_cu: Optional[List[int]],
             T: int) -> torch.Tensor:
        """n audios of T >= 1500 frames each (Whisper's 1500 + zero frames; BEATs' T_a <= T + zero frames) -> [n * n_windows(T), H_llm]."""
        w, c = self.w, self.w.cfg
        dw, db, hq = self.whisper_d, self.beats_d, c.hidden
        C = dw + (db if audio is not None else 0)
        assert C == c.enc_width, f"Q-Former encoder width {c.enc_width} != {C}"
        cat = ws.get("qf_cat", (n * T, C), BF16)
        if T == 1500:
            B.layernorm(speech, w.ln_speech_g, w.ln_speech_b, cat, 1e-5, N=dw)
        else:
            cat.zero_()                               # F.pad of the Whisper stream: frames 1500 .. T-1 are zero AFTER ln_speech
            for a in range(n):
                B.layernorm(speech[a * 1500:(a + 1) * 1500], w.ln_speech_g, w.ln_speech_b, cat[a * T:a * T + 1500], 1e-5, N=dw)
        if audio is not None:
            if T == 1500:
                cat[:, dw:].zero_()   # F.pad of the shorter BEATs stream (memset; rows past T_a stay zero)
            for a in range(n):
                ta = audio_cu[a + 1] - audio_cu[a]
                assert ta <= T
                B.layernorm(audio[audio_cu[a]:audio_cu[a] + ta], w.ln_audio_g, w.ln_audio_b,
                            cat[a * T:a * T + ta, dw:], 1e-5, N=db)
        nw = self.n_windows(T)
        W = n * nw
        h = ws.get("qf_h", (W, hq), F32)
        hb = ws.get("qf_hb", (W, hq), BF16)
        t32 = ws.get("qf_t32", (W, hq), F32)
        tb = ws.get("qf_tb", (W, hq), BF16)
        q = ws.get("qf_q", (W, hq), BF16)
        kv = ws.get("qf_kv", (n * T, 2 * hq), BF16)
        ff = ws.get("qf_ff", (W, c.ffn), BF16)
        # query token -> embeddings.LayerNorm, broadcast to every window (row stride 0 source)
        q0 = ws.get("qf_q0", (1, hq), F32)
        B.layernorm(w.query, w.emb_ln_g, w.emb_ln_b, q0, c.ln_eps)
        B.axpby_cast(q0.expand(W, hq), h)
        B.axpby_cast(q0.expand(W, hq), hb)
        for L in w.layers:
            # self-attention over ONE token: softmax == 1, context = value projection
            B.gemm(hb, L.sa_wv, tb, bias=L.sa_bv)
            B.gemm(tb, L.sa_wo, t32, bias=L.sa_bo, residual=h)
            B.layernorm(t32, L.sa_ln_g, L.sa_ln_b, h, c.ln_eps, out2=hb)
            # cross-attention: 1 query x 17 window frames
            B.gemm(hb, L.ca_wq, q, bias=L.ca_bq)
            B.gemm(cat, L.ca_wkv, kv, bias=L.ca_bkv)
            B.qformer_window_xattn(q, kv, hq, tb, n, nw, self.win, T, c.n_heads, 0.125)
            B.gemm(tb, L.ca_wo, t32, bias=L.ca_bo, residual=h)
            B.layernorm(t32, L.ca_ln_g, L.ca_ln_b, h, c.ln_eps, out2=hb)
            # query feed-forward
            B.gemm(hb, L.w1, ff, bias=L.b1, gelu=True)
            B.gemm(ff, L.w2, t32, bias=L.b2, residual=h)
            B.layernorm(t32, L.ff_ln_g, L.ff_ln_b, h, c.ln_eps, out2=hb)
        out = ws.get("qf_out", (W, self.llm_hidden), F32)
        B.gemm(hb, w.proj_w, out, bias=w.proj_b)
        return out


# ================================================================================================
# K11 decode GEMM planner: which kernel runs each GEMM of a decode step (a pure function of the batch, the model dims and the
# device's CU count, so the plan can be computed and checked without a GPU: tests/test_decode_plan.py)
# ================================================================================================
DECODE_SITES = ("qkv", "o", "gu", "down")


@dataclass(frozen=True)
class GemmLaunch:
    """One GEMM launch of a decode step.  ``tile``: the icl_gemm_args tile (0 = the library's auto choice, icl_gemm_select_tile)
    or "fp8w" (icl_gemm_fp8w); ``weight``: "row" (the row-major layer weight), "packed" (its decode-packed copy) or "fp8" (the
    fp8 decode-packed copy + row scales); ``fused_norm``: the RMSNorm after the GEMM runs in the same call (icl_gemm_rmsnorm_*)."""
    tile: object
    split_k: int
    weight: str
    N: int
    K: int
    fused_norm: bool = False


@dataclass(frozen=True)
class DecodePlan:
    Bn: int
    sites: Dict[str, GemmLaunch]    # DECODE_SITES + "lm_head"
    workspace: int                  # f32 elements of the layers' shared split-K workspace (0: no site splits)


def lm_head_tile(R: int) -> int:
    """LM head over R rows: the skinny kernel for a decode-sized batch, else the library's choice."""
    return 4 if R <= 8 else 0


def t256_split(N: int, K: int, n_cu: int) -> int:
    """Split-K of a 256-row decode GEMM on the 256x256 tile: one M-tile, ceil(N / 256) N-tiles; the slices fill ~80 % of the
    CUs (a second partial round of blocks costs more than idle CUs) and stay >= 8 K-tiles deep (the pipeline's fill / drain);
    0 = leave the GEMM on the decode tile (too few blocks either way)."""
    tiles = (N + 255) // 256
    split = min(K // 512, int(0.8 * n_cu) // tiles)
    return split if split >= 2 and tiles * split >= 0.45 * n_cu else 0


def site_shapes(cfg, k_aug: int) -> Dict[str, Tuple[int, int]]:
    """(N, K) of the four GEMM sites of a decoder layer (``k_aug``: the QKV projection's K with its LoRA columns)."""
    hd, I = cfg.hidden, cfg.ffn
    return dict(qkv=(qkv_width(cfg), k_aug), o=(hd, hd), gu=(2 * I, hd), down=(hd, I))


def decode_plan(Bn: int, cfg, k_aug: int, n_cu: int, weight_dtype: str = "bf16", decode_packed: bool = True,
                decode_t256: Sequence[str] = DECODE_SITES, fuse_norms: bool = True) -> DecodePlan:
    """The GEMM launches of one decode step over ``Bn`` rows of a Llama-family decoder (``cfg``: LlamaCfg, ``k_aug``: the QKV
    projection's K with its LoRA columns).
    Weights are streamed once per step, from decode-packed copies of the layer weights (made once, on the first decode
    step: a second 12.9 GB for Llama-2-7B — the prefill kernels keep the row-major originals; HBM is sized for both): a
    wave-load is 1 KB contiguous instead of 16 rows x 64 B.  Per layer, rotating weights: Bn <= 8 the skinny kernel
    (in-block split-K) 90-108 -> 79-87 us (5.1 TB/s at Bn = 1); 9..256 the decode tile (64-, 128- or 256-row blocks, about one
    block per CU) 115-167 -> 97-132 us at 128 rows, 214 us at 256 (0.84 vs 1.06 us per row: a weight byte serves twice the rows);
    above 256 the 64x64 LDS tile + split-K on the row-major weights."""
    hd, I = cfg.hidden, cfg.ffn

    def sk(N, K):
        tiles = ((N + 63) // 64) * ((Bn + 63) // 64)
        s = max(1, min(K // 512, (2 * n_cu + tiles - 1) // tiles))
        return min(s, 16)

    def sk5(N, K):
        return max(1, min(n_cu // ((N + 127) // 128), K // 512))
    plan = {}
    for name, (N, K) in site_shapes(cfg, k_aug).items():
        if Bn <= 8 and weight_dtype == "fp8":
            tile, split, weight = "fp8w", 1, "fp8"    # FP8 weight mode: the fp8-weight skinny kernel (tile 6's arithmetic on W')
        elif Bn <= 256 and decode_packed:
            if Bn <= 8:
                tile, split, weight = 6, 1, "packed"
            else:
                tile, split, weight = 5, sk5(N, K), "packed"
                s256 = t256_split(N, K, n_cu) if Bn > 128 and name in decode_t256 else 0
                if s256:
                    tile, split, weight = 3, s256, "row"
        elif Bn <= 8:
            tile, split, weight = 4, 1, "row"
        else:
            tile, split, weight = 2, sk(N, K), "row"
        plan[name] = GemmLaunch(tile, split, weight, N, K, fused_norm=fuse_norms and name in ("o", "down"))
    plan["lm_head"] = GemmLaunch(lm_head_tile(Bn), 1, "row", cfg.vocab, hd)
    nsplit = max(p.split_k for p in plan.values())
    return DecodePlan(Bn, plan, nsplit * Bn * max(qkv_width(cfg), 2 * I) if nsplit > 1 else 0)


def prefill_sites(cfg, k_aug: int, tile: int = 0) -> Dict[str, GemmLaunch]:
    """The four GEMM sites of a prefill layer, in the form of ``DecodePlan.sites``: the row-major weights, no split-K, the
    library's tile choice (0) — or one pinned ``tile`` (the trimmed last layer, ``LlamaHIP._last_layer_rows``)."""
    return {name: GemmLaunch(tile, 1, "row", N, K) for name, (N, K) in site_shapes(cfg, k_aug).items()}


# ================================================================================================
# K9 + K10 + K11 (+K12 host side): Llama
# ================================================================================================
class LlamaHIP:
    decode_packed_weights = True     # micro-batch <= 256: decode GEMMs stream decode-packed copies of the layer weights
    fuse_decode_norms = True         # decode: o_proj / down_proj + the RMSNorm that follows them in one call (icl_gemm_rmsnorm_bf16)
    fuse_decode_rope = os.environ.get("ICL_FUSE_DECODE_ROPE", "1") != "0"   # decode: RoPE + K/V append inside the attention launch (icl_attn_decode_rope_bf16)

    # Decode GEMMs at 129..256 rows that run on the 256x256 tile with split-K instead of the decode tile (tile 5).  Measured at the
    # Llama-2-7B shapes, 256 rows, GEMM + slab reduction (tools/decode_gemm_time.py, profiles/r04_decode_gemm_ab.txt): qkv 54.8 us on
    # the decode tile -> 46.6 (split 4); o 32.2 -> 29.5 (split 8); gate/up 79.6 -> 67.1 (split 2); down 48.5 -> 49.7 stand-alone, but
    # IN SITU (tools/ab_env.sh, four interleaved rounds: profiles/r04_decode_gemm_ab.txt) the decode phase is 2.3 ms faster with `down`
    # on the 256 tile as well (split 12) — all four.  ICL_DECODE_T256 = comma list of qkv / o / gu / down overrides ("" = decode tile only).
    decode_t256 = tuple(x for x in os.environ.get("ICL_DECODE_T256", "qkv,o,gu,down").split(",") if x)

    # Generation reads the last position of every prompt only, so the LAST decoder layer of a prefill runs its q projection,
    # attention, o_proj, norm and MLP on those rows alone (``prefill(last_rows_only=True)``; bit-identical).
    # ICL_PREFILL_LAST_ROWS=0 restores the full-height last layer + a gather, for A/B.
    prefill_last_rows = os.environ.get("ICL_PREFILL_LAST_ROWS", "1") != "0"

    def decode_plan(self, Bn: int) -> DecodePlan:
        """The GEMM launches of a decode step over Bn rows on this device, in this runtime's weight mode (``decode_plan``)."""
        return decode_plan(Bn, self.w.cfg, self.w.k_aug, self.n_cu, self.weight_dtype, self.decode_packed_weights,
                           self.decode_t256, self.fuse_decode_norms)

    def __init__(self, w: PackedLlama, device, decode_packed: Optional[bool] = None, pack_now: bool = True,
                 weight_dtype: str = "bf16"):
        """``decode_packed`` (default: the class attribute): keep a second, decode-packed layout of the layer weights (+12.9 GB
        at 7B, +25 GB at 13B).  ``pack_now=False`` defers the copy to the first decode step — forward-only users
        (``forward_logits`` / loss) then never pay for it; the default packs at load time, not inside a caller's first batch.

        ``weight_dtype="fp8"``: the opt-in FP8 weight mode (include/icl_hip.h, icl_pack_fp8_weights).  Every packed decoder GEMM
        weight (wqkv with its LoRA columns, wo, wgu, wdown) is replaced by its FP8 rounding W' (bf16) and gets an fp8 decode-packed
        copy + row scales, made here on the GPU; prefill, ``forward_logits`` and decode above 8 rows run the bf16 kernels on W'
        (the bf16 decode-packed copy is then made on first use), decode at <= 8 rows streams the fp8 copy (icl_gemm_fp8w: the
        same bits as tile 6 on W', half the bytes)."""
        if weight_dtype not in ("bf16", "fp8"):
            raise ValueError(f"weight_dtype must be 'bf16' or 'fp8', not {weight_dtype!r}")
        self.w = w
        self.device = torch.device(device)
        self.n_cu = max(B.device_cu_count(), 1)
        self.weight_dtype = weight_dtype
        if decode_packed is not None:
            self.decode_packed_weights = bool(decode_packed)
        if weight_dtype == "fp8":
            self._quantize_fp8()
        elif self.decode_packed_weights and pack_now:
            self.ensure_decode_packed()

    def _quantize_fp8(self):
        """W -> W' (new bf16 tensors: wo / wdown may share storage with the caller's checkpoint image) + L.fp8 = ((q, scales) x 4)."""
        c = self.w.cfg
        for L in self.w.layers:
            packs = []
            for name, K in (("wqkv", self.w.k_aug), ("wo", c.hidden), ("wgu", c.hidden), ("wdown", c.ffn)):
                q, s, wd = B.pack_fp8_weights(getattr(L, name), K=K)
                setattr(L, name, wd)
                packs.append((q, s))
            L.fp8 = tuple(packs)
            L.decode_packed = None

    def ensure_decode_packed(self):
        """Decode-packed copies of the layer weights (second layout of the same bytes: +12.9 GB at 7B, +25 GB at 13B)."""
        c = self.w.cfg
        for L in self.w.layers:
            if getattr(L, "decode_packed", None) is None:
                L.decode_packed = (B.pack_decode_weights(L.wqkv, K=self.w.k_aug), B.pack_decode_weights(L.wo, K=c.hidden),
                                   B.pack_decode_weights(L.wgu, K=c.hidden), B.pack_decode_weights(L.wdown, K=c.ffn))

    # ---- K9 ------------------------------------------------------------------------------------
    def embed(self, ws: Workspace, src_idx: torch.Tensor, speech: Optional[torch.Tensor], name: str = "ll_h") -> torch.Tensor:
        h = ws.get(name, (src_idx.numel(), self.w.cfg.hidden), F32)
        B.embed_gather_interleave(src_idx, self.w.embed, speech, h)
        return h

    # ---- the pieces of a decoder layer over M packed rows; prefill and decode_step write out the K/V route between them ----
    def _xn(self, ws: Workspace, L, h, M: int, tag: str, decode: bool, ready: bool = False) -> torch.Tensor:
        """The layer's input for the QKV projection, bf16 [M, k_aug] in ``tag + "xn"``: RMSNorm of ``h`` (unless ``ready``: the
        previous down_proj has written it, fused into its reduction) and the LoRA down-projection into the augmentation columns."""
        c, hd = self.w.cfg, self.w.cfg.hidden
        xn = ws.get(tag + "xn", (M, self.w.k_aug), BF16, zero=True)   # augmentation tail stays zero
        if not ready:
            B.rmsnorm(h, L.rms1, xn, c.rms_eps, N=hd)
        if L.lora_a is not None:   # x_aug[:, hd:hd+2r] = x @ (s*A)^T : a skinny GEMM for prefill, a GEMV-style kernel for decode
            # prefill: always the 64x64 tile (the choice must not depend on the batch, or rows would not be batch-invariant);
            # decode: the skinny kernel (one block, K split over its 8 waves) up to 64 rows, the block-per-row kernel above
            # that (an N = 16 GEMM on the 64x64 tile is 2 blocks walking all of K: 40 us vs 15)
            r2 = L.lora_a.shape[0]
            if decode and M > 64:
                B.lora_down(xn, hd, L.lora_a, r2, 1.0, M=M)      # the LoRA scale is folded into lora_a at pack time
            else:
                B.gemm(xn, L.lora_a, xn[:, hd:hd + r2], K=hd, tile=4 if decode else 2)
        return xn

    def _site_gemm(self, L, sites: Dict[str, GemmLaunch], name: str, a, out, wsk, norm=None, **epilogue):
        """The GEMM of site ``name`` on the weight form its launch names: row-major, decode-packed (tiles 5 / 6) or the fp8
        decode-packed copy + row scales (FP8 weight mode, <= 8 rows).  ``wsk``: the split-K workspace or None;
        ``norm`` = (gamma, xn): the RMSNorm fused behind the GEMM (icl_gemm_rmsnorm_*)."""
        p, idx = sites[name], DECODE_SITES.index(name)
        q, scale = L.fp8[idx] if p.weight == "fp8" else (None, None)
        wt = q if p.weight == "fp8" else L.decode_packed[idx] if p.weight == "packed" else (L.wqkv, L.wo, L.wgu, L.wdown)[idx]
        kw = dict(split_k=p.split_k, workspace=wsk, tile=p.tile, N=p.N, K=p.K, w_scale=scale, **epilogue)
        if norm is not None:
            return B.gemm_rmsnorm(a, wt, out, norm[0], self.w.cfg.rms_eps, norm[1], **kw)
        return B.gemm(a, wt, out, **kw)

    def _attn_out_mlp(self, ws: Workspace, L, h, xn, att, tag: str, sites: Dict[str, GemmLaunch], wsk, next_norm=None) -> bool:
        """From the attention output to the end of the layer: h += att Wo^T, post-attention RMSNorm into ``xn``, gate/up, h += down.
        ``next_norm`` = (gamma, out bf16 [M, >= hidden]) of the RMSNorm that follows this layer (the next layer's input norm, or
        the final norm): a ``down`` launch with ``fused_norm`` runs it in its split-K reduction, as ``o`` does the post-attention
        norm (icl_gemm_rmsnorm_bf16) — True is returned when it has been written."""
        c = self.w.cfg
        act = ws.get(tag + "act", (att.shape[0], c.ffn), BF16)
        if sites["o"].fused_norm:     # one call (one kernel when the GEMM is split-K)
            self._site_gemm(L, sites, "o", att, h, wsk, norm=(L.rms2, xn), residual=h)
        else:
            self._site_gemm(L, sites, "o", att, h, wsk, residual=h)
            B.rmsnorm(h, L.rms2, xn, c.rms_eps, N=c.hidden)
        self._site_gemm(L, sites, "gu", xn, act, wsk, swiglu=True)
        if sites["down"].fused_norm and next_norm is not None:
            self._site_gemm(L, sites, "down", act, h, wsk, norm=next_norm, residual=h)
            return True
        self._site_gemm(L, sites, "down", act, h, wsk, residual=h)
        return False

    # ---- K10: prefill over ragged packed sequences ------------------------------------------------
    def prefill(self, ws: Workspace, h: torch.Tensor, seq_lens: List[int], cache: Optional["KVCache"] = None,
                last_rows_only: bool = False, last_out: Optional[torch.Tensor] = None, probes=None) -> torch.Tensor:
        """h f32 [sum S_b, hidden] (modified in place) -> same buffer holding the final hidden states.

        ``probes`` (a ``probes.Probes``; needs ``last_rows_only``, and a bf16 cache where it reads one): what is read and
        written at the sequences' LAST rows.  The layers call it at three points and launch what they launch otherwise:
        ``residual_site(l, h)`` at the top of layer l, before its input norm and before the branch into the trimmed last layer —
        so that layer's k / v of the row see a rewritten stream — and, as site n_layers, on the gathered rows before they are
        returned; ``keys_appended`` once q / k are rotated and k is in the cache, in front of the attention launch;
        ``attention_written`` after the layer's attention launch, when the cache holds every prompt position in every prefill
        form — it may rewrite the last rows of ``att``, every other row keeps its bits.

        ``last_rows_only`` (needs a cache): return only the final hidden state of the LAST row of every sequence, f32
        [len(seq_lens), hidden] (written into ``last_out`` when given) — what generation feeds to the final norm and the LM
        head.  Every layer's K / V still reach the cache for all rows; ``h`` is then NOT the final hidden states (the last
        layer leaves its other rows untouched, ``_last_layer_rows``).  The rows returned are bit-identical to the same rows of
        the full prefill."""
        c, w = self.w.cfg, self.w
        dev = h.device
        M = sum(seq_lens)
        cu_h = [0]
        for s in seq_lens:
            cu_h.append(cu_h[-1] + s)
        assert max(seq_lens) <= c.max_pos
        assert cache is not None or not last_rows_only, "prefill(last_rows_only=True) needs a KV cache"
        pos = _i32([p for s in seq_lens for p in range(s)], dev)
        sid = _i32([b for b, s in enumerate(seq_lens) for _ in range(s)], dev)
        cu = _i32(cu_h, dev)
        maxS = max(seq_lens)
        H, D, hd = c.n_heads, c.head_dim, c.hidden
        k_off, v_off = qkv_offsets(c)
        gqa = c.group > 1      # grouped-query attention: no fused RoPE epilogue, so k / v stay packed next to q and no trimming
        qkn = c.qk_norm        # per-head q / k RMSNorm (Qwen3) in front of the rotation: one more reason not to fuse or trim
        fp8 = cache is not None and cache.dtype == "fp8"
        max_len = cache.max_len if cache is not None else 0
        # the QKV GEMM runs on the 256x256 tile: RoPE + cache append run in its staged epilogue (same bits as the two calls)
        epilogue = not gqa and not qkn and B.rope_fusable(M, H, D, w.k_aug)
        in_cache = epilogue and cache is not None and not fp8      # ... and the attention reads k / v from the (bf16) cache
        # the trimmed last layer is built on the 256-tile's fused RoPE epilogue (head_dim 128) and a bf16 cache; other models
        # and the FP8 KV mode (whose prefill attends to unrounded packed k / v) keep the full-height layer and gather after it
        trim = (last_rows_only and self.prefill_last_rows and not fp8 and not gqa and not qkn
                and B.rope_epilogue_ok(H, D, w.k_aug) and not (probes is not None and probes.reads_every_row))
        last_idx = out = None
        if last_rows_only:
            last_idx = _i32([e - 1 for e in cu_h[1:]], dev)
            out = last_out if last_out is not None else ws.get("pfl_h", (len(seq_lens), hd), F32)
        sites = prefill_sites(c, w.k_aug)
        if probes is not None:
            probes.start_prefill(seq_lens, cu_h, last_idx, cache)      # its preconditions and its host tables of this call
        for i, L in enumerate(w.layers):
            if probes is not None:
                probes.residual_site(i, h, packed=True)
            kc, vc, ks, vs = cache.layer(i) if cache is not None else (None, None, None, None)
            if trim and i == len(w.layers) - 1:
                hg = self._last_layer_rows(ws, L, h, seq_lens, pos, sid, cu, kc, vc, max_len, last_idx, out, probes=probes)
                break
            xn = self._xn(ws, L, h, M, "pf_", decode=False)
            qkv = ws.get("pf_qkv", (M, qkv_width(c)), BF16)
            att = ws.get("pf_att", (M, hd), BF16)
            # Who rotates q / k and where k / v go.  With a bf16 cache and the fused epilogue, k / v are written ONCE — into the
            # cache — and the attention reads them there ([seq][head][pos][D]: 256-B rows at a 256-B stride instead of a 3*hidden
            # stride); the k / v columns of the QKV buffer are never written.  Otherwise they stay packed next to q.  FP8 KV
            # cache: prefill attends to its own unrounded k / v, so RoPE appends nowhere and one icl_kv_append_fp8 pass rounds the
            # rows into the cache before the attention.
            if in_cache:            # epilogue into the cache
                B.gemm(xn, L.wqkv, qkv, bias=L.bqkv, tile=3,
                       rope=(k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H, D, max_len, False))
            elif epilogue:          # epilogue with packed k / v: no cache (teacher-forced forward) or the FP8 one
                B.gemm(xn, L.wqkv, qkv, bias=L.bqkv, tile=3,
                       rope=(k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, None, None, H, D, 0, True))
            elif qkn:               # per-head q / k norm + RoPE + append in one launch, multi-head or grouped (never the FP8 cache)
                self._site_gemm(L, sites, "qkv", xn, qkv, None, bias=L.bqkv)
                B.qknorm_rope_kv(qkv, k_off, v_off, L.q_gamma, L.k_gamma, c.rms_eps, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H,
                                 c.kv_heads, D, max_len, M=M)
            elif gqa:               # stand-alone RoPE + append, grouped-query (never with the FP8 cache)
                self._site_gemm(L, sites, "qkv", xn, qkv, None, bias=L.bqkv)
                B.rope_kv_gqa(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H, c.kv_heads, D, max_len, M=M)
            elif fp8:               # stand-alone RoPE, no append
                self._site_gemm(L, sites, "qkv", xn, qkv, None, bias=L.bqkv)
                B.rope_kv(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, None, None, H, D, 0, M=M)
            else:                   # stand-alone RoPE + append to the bf16 cache, if there is one
                self._site_gemm(L, sites, "qkv", xn, qkv, None, bias=L.bqkv)
                B.rope_kv(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H, D, max_len, M=M)
            if fp8:
                B.kv_append_fp8(qkv, k_off, v_off, pos, sid, kc, vc, ks, vs, H, D, max_len, M=M)
            if probes is not None:      # the last rows of the QKV buffer are the deciding queries; their keys are in the cache by now
                probes.keys_appended(i, qkv[:, :k_off], kc, c, max_len, packed=True)
            if in_cache:
                B.attn_fwd(qkv[:, :hd], kc, vc, att, cu, maxS, H, D, D ** -0.5, causal=True, kv_cache_max_len=max_len)
            else:
                B.attn_fwd(qkv[:, :k_off], qkv[:, k_off:v_off], qkv[:, v_off:], att, cu, maxS, H, D, D ** -0.5, causal=True,
                           n_kv_heads=c.kv_heads if gqa else 0)
            if probes is not None:
                probes.attention_written(i, qkv[:, :k_off], att, kc, vc, c, max_len, packed=True)
            self._attn_out_mlp(ws, L, h, xn, att, "pf_", sites, None)
        else:
            hg = B.gather_rows(h, last_idx, out) if last_rows_only else h
        if probes is not None:          # gathered row b is sequence b's
            probes.residual_site(len(w.layers), hg)
        return hg

    def _last_layer_rows(self, ws: Workspace, L, h, seq_lens: List[int], pos, sid, cu, kc, vc, max_len: int,
                         last_idx, hg, probes=None) -> torch.Tensor:
        """The last decoder layer of a prefill whose caller reads the last row of every sequence only: the layer's k / v are
        projected (and appended to the cache) for all M rows; q, the attention, o_proj, the post-attention norm and the MLP run
        on the len(seq_lens) gathered rows.  Exact, not approximate: every kernel here computes a row independently of its
        neighbours, and each gathered row goes through the arithmetic the full-height layer gives it — the 256x256 tile's K
        order (tiles 1 - 3 agree, so the small launches are pinned to tile 3 instead of the library's small-M choice), the same
        fused RoPE epilogue at the row's position, and the full attention launch's wave, lane and 64-key tile sequence
        (icl_attn_fwd_suffix_bf16, q_len = 1).  The gathered buffers have names of their own (pfl_*): the full-height ones
        keep their size.  ``probes``: ``prefill``'s, called on the gathered rows — row b is sequence b's — at the same two points
        around the attention launch.  Returns ``hg``, f32 [len(seq_lens), hidden]: the rows' final hidden states."""
        c, w = self.w.cfg, self.w
        hd, D, H = c.hidden, c.head_dim, c.n_heads
        M, Bn, dev = sum(seq_lens), len(seq_lens), h.device
        xn = self._xn(ws, L, h, M, "pf_", decode=False)
        rope = (w.rope_cos, w.rope_sin)
        # k | v rows of wqkv, all M rows, into the cache only: C is never written (kv_rows_to_c = 0)
        qkv = ws.get("pf_qkv", (M, qkv_width(c)), BF16)
        B.gemm(xn, L.wqkv[hd:], qkv, bias=L.bqkv[hd:] if L.bqkv is not None else None, tile=3,
               rope=(0, hd, *rope, pos, sid, kc, vc, H, D, max_len, False))
        B.gather_rows(h, last_idx, hg)
        xg = ws.get("pfl_xn", (Bn, w.k_aug), BF16)              # whole augmented rows: the LoRA columns and the zero tail come along
        B.gather_rows(xn, last_idx, xg)
        # q rows of wqkv on the gathered rows, rotated at each row's own (last) position
        q = ws.get("pfl_q", (Bn, hd), BF16)
        B.gemm(xg, L.wqkv[:hd], q, bias=L.bqkv[:hd] if L.bqkv is not None else None, tile=3,
               rope=(hd, hd, *rope, _i32([s - 1 for s in seq_lens], dev), None, None, None, H, D, max_len))
        if probes is not None:
            probes.keys_appended(len(w.layers) - 1, q, kc, c, max_len)
        att = ws.get("pfl_att", (Bn, hd), BF16)
        B.attn_fwd(q, kc, vc, att, cu, max(seq_lens), H, D, D ** -0.5, causal=True, kv_cache_max_len=max_len,
                   cu_q=_i32(list(range(Bn + 1)), dev))
        if probes is not None:
            probes.attention_written(len(w.layers) - 1, q, att, kc, vc, c, max_len)
        self._attn_out_mlp(ws, L, hg, xg, att, "pfl_", prefill_sites(c, w.k_aug, tile=3), None)
        return hg

    def logits(self, ws: Workspace, h_rows: torch.Tensor, name: str = "ll_logits", xn_ready: bool = False) -> torch.Tensor:
        """h_rows f32 [R, hidden] -> logits f32 [R, vocab] (final RMSNorm + lm_head).  ``xn_ready``: the final norm has been
        written into ``name + "_xn"`` already (decode: fused into the last down_proj's reduction)."""
        c = self.w.cfg
        R = h_rows.shape[0]
        xn = ws.get(name + "_xn", (R, c.hidden), BF16)
        out = ws.get(name, (R, c.vocab), F32)
        if not xn_ready:
            B.rmsnorm(h_rows, self.w.norm, xn, c.rms_eps)
        B.gemm(xn, self.w.lm_head, out, tile=lm_head_tile(R))
        return out

    # ---- K11: one decode step for Bn sequences -----------------------------------------------------
    def decode_step(self, ws: Workspace, cache: "KVCache", next_ids: torch.Tensor, pos: torch.Tensor,
                    lens: torch.Tensor, sid: torch.Tensor, probes=None) -> torch.Tensor:
        """``probes`` (a ``probes.Probes``, the decode steps' bundle): ``residual_site(l, h)`` at the top of layer l (n_layers: in
        front of the final norm) says whether it rewrote rows of ``h``.  The previous layer's ``down`` launch may have written
        this layer's normed input from the unwritten ``h``, so the layer then runs its input norm as a launch of its own (site
        n_layers: the final norm).  ``attention_written`` after a layer's attention launch may rewrite rows of the attention
        output from the rotated q.  When ``masks_attention`` says it will, the step takes the two-launch RoPE + attention form
        at every batch size — the fused launch leaves q unrotated in ``qkv``; the two forms are bit-identical — so the other rows
        keep their bits."""
        c, w = self.w.cfg, self.w
        Bn = next_ids.numel()
        h = self.embed(ws, next_ids, None, name="dc_h")
        H, D = c.n_heads, c.head_dim
        k_off, v_off = qkv_offsets(c)
        plan = self.decode_plan(Bn)
        sites = plan.sites
        if any(p.weight == "packed" for p in sites.values()):
            self.ensure_decode_packed()

        layers = w.layers
        xn_next = ws.get("dc_xn", (Bn, w.k_aug), BF16, zero=True)            # the layers' normalised-input buffer (_xn's)
        xn_final = ws.get("dc_logits_xn", (Bn, c.hidden), BF16)
        qkv = ws.get("dc_qkv", (Bn, qkv_width(c)), BF16)
        att = ws.get("dc_att", (Bn, c.hidden), BF16)
        wsk = ws.get("dc_splitk", (plan.workspace,), F32) if plan.workspace else None
        fp8 = cache.dtype == "fp8"
        max_len, scale = cache.max_len, D ** -0.5
        # One launch: rotate q / k at pos, append k / v, attend — bit-identical to the two launches, so the choice is free.
        # Same-box A/B (tools/ab_decode_rope.sh, profiles/r04_decode_rope_ab.txt): at 256 rows decode 143.2 -> 142.5 ms; at ONE
        # sequence 58.4 -> 59.6 ms per utterance — the rotation's dependent loads (pos -> cos / sin, q, k) sit in front of a
        # latency-bound attention and cost more than the 5-us launch they replace — so small batches keep the two launches.
        masked = probes is not None and probes.masks_attention(cache)
        fuse_rope = self.fuse_decode_rope and Bn > 8 and not c.qk_norm and not masked
        ready = False
        for i, L in enumerate(layers):
            kc, vc, ks, vs = cache.layer(i)
            if probes is not None and probes.residual_site(i, h):
                ready = False       # what the previous down wrote is the norm of the rows as they were
            xn = self._xn(ws, L, h, Bn, "dc_", decode=True, ready=ready)
            self._site_gemm(L, sites, "qkv", xn, qkv, wsk, bias=L.bqkv)
            if c.qk_norm:         # QK-norm (Qwen3): two launches at every batch size, norm + RoPE + append and the decode attention
                B.qknorm_rope_kv(qkv, k_off, v_off, L.q_gamma, L.k_gamma, c.rms_eps, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H,
                                 c.kv_heads, D, max_len, M=Bn)
                if c.group > 1:
                    B.attn_decode_gqa(qkv[:, :k_off], kc, vc, att, lens, H, c.kv_heads, D, max_len, scale)
                else:
                    B.attn_decode(qkv[:, :k_off], kc, vc, att, lens, H, D, max_len, scale)
            elif c.group > 1:     # grouped-query attention: two launches at every batch size, RoPE + append and the GQA decode attention
                B.rope_kv_gqa(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H, c.kv_heads, D, max_len, M=Bn)
                B.attn_decode_gqa(qkv[:, :k_off], kc, vc, att, lens, H, c.kv_heads, D, max_len, scale)
            elif fp8 and fuse_rope:   # FP8 KV cache: the same two forms, rounding the appended row to x' (icl_hip.h)
                B.attn_decode_rope_fp8(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, ks, vs, att, lens, H, D,
                                       max_len, scale)
            elif fp8:
                B.rope_kv_fp8(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, ks, vs, H, D, max_len, M=Bn)
                B.attn_decode_fp8(qkv[:, :k_off], kc, vc, ks, vs, att, lens, H, D, max_len, scale)
            elif fuse_rope:
                B.attn_decode_rope(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, att, lens, H, D, max_len, scale)
            else:
                B.rope_kv(qkv, k_off, v_off, w.rope_cos, w.rope_sin, pos, sid, kc, vc, H, D, max_len, M=Bn)
                B.attn_decode(qkv[:, :k_off], kc, vc, att, lens, H, D, max_len, scale)
            if probes is not None:
                probes.attention_written(i, qkv[:, :k_off], att, kc, vc, c, max_len, lens=lens)
            nxt = (layers[i + 1].rms1, xn_next) if i + 1 < len(layers) else (w.norm, xn_final)
            ready = self._attn_out_mlp(ws, L, h, xn, att, "dc_", sites, wsk, next_norm=nxt)
        if probes is not None and probes.residual_site(len(layers), h):
            ready = False
        return self.logits(ws, h, name="dc_logits", xn_ready=ready)


KV_DTYPES = ("bf16", "fp8")


def check_kv_dtype(value: str, cfg=None) -> str:
    """The KV-cache dtype of the LLM decoder: "bf16" (default) or "fp8" (the opt-in FP8 KV cache, include/icl_hip.h).
    ``cfg`` (the decoder's LlamaCfg, when known): the FP8 KV cache has no grouped-query kernels and none with the per-head q / k
    norm of a QK-norm decoder (Qwen3) — "fp8" is then a ValueError."""
    if value not in KV_DTYPES:
        raise ValueError(f"llm_kv_dtype must be one of {KV_DTYPES}, not {value!r}")
    if value == "fp8" and cfg is not None and getattr(cfg, "group", 1) > 1:
        raise ValueError("llm_kv_dtype='fp8' is not available for a grouped-query decoder "
                         f"({cfg.n_heads} query heads / {cfg.kv_heads} K/V heads): the FP8 KV kernels are multi-head only")
    if value == "fp8" and cfg is not None and getattr(cfg, "qk_norm", False):
        raise ValueError("llm_kv_dtype='fp8' is not available for a QK-norm decoder (qk_norm=True, Qwen3): the FP8 KV kernels "
                         "have no per-head q / k RMSNorm in front of the rotation")
    return value


class KVCache:
    """K/V cache, per layer [n_seqs][kv_heads][max_len][head_dim] (one contiguous stream per (seq, K/V head); kv_heads = n_heads
    unless the decoder uses grouped-query attention): a view of
    the workspace's single ``kv_k`` / ``kv_v`` allocations, which grow to the largest (n_seqs x max_len) seen.

    ``dtype="fp8"`` (the opt-in FP8 KV cache, include/icl_hip.h): ``k`` / ``v`` hold the e4m3fn bytes of every row (uint8, the
    same shape) and ``ks`` / ``vs`` its f32 scale 2^e, [n_layers][n_seqs][n_heads][max_len]; all four keep the ``kv_`` prefix,
    so captured decode graphs are retired when they move (Workspace.GRAPH_VISIBLE)."""

    def __init__(self, cfg, n_seqs: int, max_len: int, ws: Workspace, dtype: str = "bf16"):
        self.n_seqs, self.max_len, self.dtype = n_seqs, max_len, check_kv_dtype(dtype, cfg)
        kv_heads = getattr(cfg, "kv_heads", cfg.n_heads)       # (a cfg-like object without grouped-query attention: n_heads)
        shape = (cfg.n_layers, n_seqs, kv_heads, max_len, cfg.head_dim)
        if dtype == "fp8":
            self.k = ws.get("kv_k8", shape, torch.uint8)
            self.v = ws.get("kv_v8", shape, torch.uint8)
            self.ks = ws.get("kv_ks", shape[:4], F32)
            self.vs = ws.get("kv_vs", shape[:4], F32)
        else:
            self.k = ws.get("kv_k", shape, BF16)
            self.v = ws.get("kv_v", shape, BF16)
            self.ks = self.vs = None

    def layer(self, i: int):
        """(k, v, k scales, v scales) of layer i; the scales are None in a bf16 cache."""
        return self.k[i], self.v[i], None if self.ks is None else self.ks[i], None if self.vs is None else self.vs[i]

    def planes(self):
        """((k, k scales), (v, v scales)); the scales are None in a bf16 cache."""
        return ((self.k, self.ks), (self.v, self.vs))

    def rows(self, b0: int, b1: int) -> "KVCache":
        """The cache of sequences b0 .. b1-1 only (views; sequence ids inside are relative to b0): a prefill over a chunk of
        the batch appends into, and reads from, its own block of the one allocation."""
        sub = object.__new__(KVCache)
        sub.n_seqs, sub.max_len, sub.dtype = b1 - b0, self.max_len, self.dtype
        sub.k, sub.v = self.k[:, b0:b1], self.v[:, b0:b1]
        sub.ks, sub.vs = (self.ks[:, b0:b1], self.vs[:, b0:b1]) if self.ks is not None else (None, None)
        return sub
