#!/usr/bin/env python3
"""Generates tests/golden/qwen3_tiny.npz: the pin of the QK-norm decoder oracle (tests/qknorm_ref.py QKNormOracle) to the
installed transformers' Qwen3ForCausalLM, fp32 on the CPU.

The model: 2 layers, 2 query heads / 1 K/V head, head_dim 128 (hidden 256), FFN 64, vocabulary 48, rms_norm_eps 1e-6, no
biases, untied embeddings.  Matrices are N(0, 0.02) x 3, the per-head norm gains 1 + 0.3 N(0, 1) (q and k apart), the other
norm gains 1 + 0.1 N(0, 1); every weight is rounded to bf16 before the run and stored as its bf16 bit pattern (uint16), so the
fp32 model and the file hold the same numbers.  Stored next to the weights: inputs_embeds [2, 13, 256], the logits, labels and
the HF cross-entropy loss, and 8 greedy ids per row.
Usage:  python tests/golden/make_qwen3_golden.py
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=64,
           vocab_size=48, rms_norm_eps=1e-6, max_position_embeddings=128, rope_theta=10000.0, attention_bias=False,
           tie_word_embeddings=False)
NEW = 8


def main():
    from transformers import Qwen3Config, Qwen3ForCausalLM
    torch.manual_seed(11)
    m = Qwen3ForCausalLM(Qwen3Config(**CFG)).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * 0.06)
            elif name.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(1.0 + 0.3 * torch.randn_like(p))
            else:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            p.copy_(p.to(torch.bfloat16).float())
        emb = torch.randn(2, 13, CFG["hidden_size"]) * 0.5
        labels = torch.full((2, 13), -100)
        labels[:, -5:] = torch.randint(0, CFG["vocab_size"], (2, 5))
        out = m(inputs_embeds=emb, labels=labels)
        ids = m.generate(inputs_embeds=emb, attention_mask=torch.ones(2, 13, dtype=torch.long), max_new_tokens=NEW, do_sample=False,
                         num_beams=1, pad_token_id=CFG["vocab_size"] - 1, eos_token_id=None)
    weights = {"w:" + k: v.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16) for k, v in m.state_dict().items()}
    path = os.path.join(HERE, "qwen3_tiny.npz")
    np.savez_compressed(path, emb=emb.numpy(), logits=out.logits.numpy(), labels=labels.numpy(), loss=out.loss.numpy(),
                        gen=ids.numpy(), **weights)
    print(f"qwen3_tiny.npz: {os.path.getsize(path) / 1024:.1f} KiB, max |logit| {float(out.logits.abs().max()):.2f}, "
          f"loss {float(out.loss):.4f}, ids {ids.tolist()}")


if __name__ == "__main__":
    main()
