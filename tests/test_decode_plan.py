"""The decode-step GEMM plan (runtime/engines.py: decode_plan) at the real model dims, on the CPU: every launch it plans passes
the library's argument checks (gemm.hip), and the plan itself is pinned, so a change to the planner has to update the table
below on purpose.  tests/test_gpu_decode_plan.py runs these same launches on the GPU against an fp64 reference."""
import pytest

from icl_speech_text_llm_amd.runtime import engines as E
from icl_speech_text_llm_amd.runtime.config import QwenAudioCfg, SalmonnCfg
from icl_speech_text_llm_amd.runtime.packing import llama_k_aug

N_CU = 256                  # MI355X
MODELS = {"llama2_7b": SalmonnCfg.llama2_7b().llama, "llama2_13b": SalmonnCfg.llama2_13b().llama, "qwen2_7b": QwenAudioCfg().llm}
BATCHES = (1, 8, 9, 64, 65, 128, 129, 255, 256, 257)
CASES = [(m, bn, wd, dp) for m in MODELS for wd in ("bf16", "fp8") for dp in (True, False) for bn in BATCHES]


def _plan(model, Bn, wd, dp, **kw):
    cfg = MODELS[model]
    return E.decode_plan(Bn, cfg, llama_k_aug(cfg), N_CU, wd, dp, **kw)


def test_model_dims():
    """The dims the table is pinned at (LoRA-augmented QKV K, vocab with SALMONN's added pad token / Qwen2-Audio's)."""
    got = {m: (c.hidden, c.ffn, llama_k_aug(c), c.vocab, c.qkv_bias) for m, c in MODELS.items()}
    assert got == {"llama2_7b": (4096, 11008, 4160, 32001, False), "llama2_13b": (5120, 13824, 5184, 32001, False),
                   "qwen2_7b": (4096, 11008, 4160, 156032, True)}


@pytest.mark.parametrize("model,Bn,wd,dp", CASES)
def test_plan_passes_the_library_argument_checks(model, Bn, wd, dp):
    cfg = MODELS[model]
    plan = _plan(model, Bn, wd, dp)
    assert plan.Bn == Bn and set(plan.sites) == set(E.DECODE_SITES) | {"lm_head"}
    shapes = dict(qkv=(3 * cfg.hidden, llama_k_aug(cfg)), o=(cfg.hidden, cfg.hidden), gu=(2 * cfg.ffn, cfg.hidden),
                  down=(cfg.hidden, cfg.ffn), lm_head=(cfg.vocab, cfg.hidden))
    for name, g in plan.sites.items():
        assert (g.N, g.K) == shapes[name], name
        assert g.K % 64 == 0
        assert 1 <= g.split_k <= min(g.K // 64, 64), (name, g)
        if g.tile == 3:
            assert g.K // g.split_k >= 128 and g.N % 4 == 0, (name, g)
        if g.tile in (4, 6, "fp8w"):                # the skinny kernels: M <= 64, K split inside the block
            assert Bn <= 64 and g.split_k == 1, (name, g)
        if g.tile == 5:
            assert Bn <= 256, (name, g)
        if g.split_k > 1:                           # one workspace serves every site of the layer
            assert plan.workspace >= g.split_k * Bn * g.N, (name, g, plan.workspace)
        # the weight form follows the kernel: tiles 5 / 6 read the decode-packed copy, fp8w the fp8 one, the rest the original
        want = {5: "packed", 6: "packed", "fp8w": "fp8"}.get(g.tile, "row")
        assert g.weight == want, (name, g)
        assert g.tile != "fp8w" or wd == "fp8"
        assert g.weight != "packed" or dp
        assert g.fused_norm == (name in ("o", "down")), (name, g)
        if g.fused_norm:                            # icl_gemm_rmsnorm_*: N % 4 == 0, N <= 8192
            assert g.N % 4 == 0 and g.N <= 8192
    if max(g.split_k for g in plan.sites.values()) == 1:
        assert plan.workspace == 0
    lm = plan.sites["lm_head"]
    assert (lm.tile == 4) == (Bn <= 8) and lm.tile in (0, 4) and lm.split_k == 1 and lm.weight == "row"
    assert E.lm_head_tile(Bn) == lm.tile


# (model, Bn, weight dtype, decode-packed) -> "qkv o gu down" as tile/split + weight form (p packed, r row-major, f fp8),
# the LM head's tile (0 = the library's choice) and the split-K workspace in f32 elements; n_cu = 256.
PINNED = {
    # llama2_7b
    ("llama2_7b", 1, "bf16", True): "6/1p 6/1p 6/1p 6/1p lm=4 ws=0",
    ("llama2_7b", 8, "bf16", True): "6/1p 6/1p 6/1p 6/1p lm=4 ws=0",
    ("llama2_7b", 9, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=1585152",
    ("llama2_7b", 64, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11272192",
    ("llama2_7b", 65, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11448320",
    ("llama2_7b", 128, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=22544384",
    ("llama2_7b", 129, "bf16", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=34080768",
    ("llama2_7b", 255, "bf16", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67368960",
    ("llama2_7b", 256, "bf16", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67633152",
    ("llama2_7b", 257, "bf16", True): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    ("llama2_7b", 1, "bf16", False): "4/1r 4/1r 4/1r 4/1r lm=4 ws=0",
    ("llama2_7b", 8, "bf16", False): "4/1r 4/1r 4/1r 4/1r lm=4 ws=0",
    ("llama2_7b", 9, "bf16", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=1585152",
    ("llama2_7b", 64, "bf16", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=11272192",
    ("llama2_7b", 65, "bf16", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=5724160",
    ("llama2_7b", 128, "bf16", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=11272192",
    ("llama2_7b", 129, "bf16", False): "2/1r 2/3r 2/1r 2/3r lm=0 ws=8520192",
    ("llama2_7b", 255, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11228160",
    ("llama2_7b", 256, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11272192",
    ("llama2_7b", 257, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    ("llama2_7b", 1, "fp8", True): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_7b", 8, "fp8", True): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_7b", 9, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=1585152",
    ("llama2_7b", 64, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11272192",
    ("llama2_7b", 65, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11448320",
    ("llama2_7b", 128, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=22544384",
    ("llama2_7b", 129, "fp8", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=34080768",
    ("llama2_7b", 255, "fp8", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67368960",
    ("llama2_7b", 256, "fp8", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67633152",
    ("llama2_7b", 257, "fp8", True): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    ("llama2_7b", 1, "fp8", False): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_7b", 8, "fp8", False): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_7b", 9, "fp8", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=1585152",
    ("llama2_7b", 64, "fp8", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=11272192",
    ("llama2_7b", 65, "fp8", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=5724160",
    ("llama2_7b", 128, "fp8", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=11272192",
    ("llama2_7b", 129, "fp8", False): "2/1r 2/3r 2/1r 2/3r lm=0 ws=8520192",
    ("llama2_7b", 255, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11228160",
    ("llama2_7b", 256, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11272192",
    ("llama2_7b", 257, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    # llama2_13b
    ("llama2_13b", 1, "bf16", True): "6/1p 6/1p 6/1p 6/1p lm=4 ws=0",
    ("llama2_13b", 8, "bf16", True): "6/1p 6/1p 6/1p 6/1p lm=4 ws=0",
    ("llama2_13b", 9, "bf16", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=1492992",
    ("llama2_13b", 64, "bf16", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=10616832",
    ("llama2_13b", 65, "bf16", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=10782720",
    ("llama2_13b", 128, "bf16", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=21233664",
    ("llama2_13b", 129, "bf16", True): "3/3r 3/10r 5/1p 3/10r lm=0 ws=35665920",
    ("llama2_13b", 255, "bf16", True): "3/3r 3/10r 5/1p 3/10r lm=0 ws=70502400",
    ("llama2_13b", 256, "bf16", True): "3/3r 3/10r 5/1p 3/10r lm=0 ws=70778880",
    ("llama2_13b", 257, "bf16", True): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14211072",
    ("llama2_13b", 1, "bf16", False): "4/1r 4/1r 4/1r 4/1r lm=4 ws=0",
    ("llama2_13b", 8, "bf16", False): "4/1r 4/1r 4/1r 4/1r lm=4 ws=0",
    ("llama2_13b", 9, "bf16", False): "2/3r 2/7r 2/2r 2/7r lm=0 ws=1741824",
    ("llama2_13b", 64, "bf16", False): "2/3r 2/7r 2/2r 2/7r lm=0 ws=12386304",
    ("llama2_13b", 65, "bf16", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=7188480",
    ("llama2_13b", 128, "bf16", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=14155776",
    ("llama2_13b", 129, "bf16", False): "2/1r 2/3r 2/1r 2/3r lm=0 ws=10699776",
    ("llama2_13b", 255, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14100480",
    ("llama2_13b", 256, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14155776",
    ("llama2_13b", 257, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14211072",
    ("llama2_13b", 1, "fp8", True): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_13b", 8, "fp8", True): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_13b", 9, "fp8", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=1492992",
    ("llama2_13b", 64, "fp8", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=10616832",
    ("llama2_13b", 65, "fp8", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=10782720",
    ("llama2_13b", 128, "fp8", True): "5/2p 5/6p 5/1p 5/6p lm=0 ws=21233664",
    ("llama2_13b", 129, "fp8", True): "3/3r 3/10r 5/1p 3/10r lm=0 ws=35665920",
    ("llama2_13b", 255, "fp8", True): "3/3r 3/10r 5/1p 3/10r lm=0 ws=70502400",
    ("llama2_13b", 256, "fp8", True): "3/3r 3/10r 5/1p 3/10r lm=0 ws=70778880",
    ("llama2_13b", 257, "fp8", True): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14211072",
    ("llama2_13b", 1, "fp8", False): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_13b", 8, "fp8", False): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("llama2_13b", 9, "fp8", False): "2/3r 2/7r 2/2r 2/7r lm=0 ws=1741824",
    ("llama2_13b", 64, "fp8", False): "2/3r 2/7r 2/2r 2/7r lm=0 ws=12386304",
    ("llama2_13b", 65, "fp8", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=7188480",
    ("llama2_13b", 128, "fp8", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=14155776",
    ("llama2_13b", 129, "fp8", False): "2/1r 2/3r 2/1r 2/3r lm=0 ws=10699776",
    ("llama2_13b", 255, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14100480",
    ("llama2_13b", 256, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14155776",
    ("llama2_13b", 257, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=14211072",
    # qwen2_7b
    ("qwen2_7b", 1, "bf16", True): "6/1p 6/1p 6/1p 6/1p lm=4 ws=0",
    ("qwen2_7b", 8, "bf16", True): "6/1p 6/1p 6/1p 6/1p lm=4 ws=0",
    ("qwen2_7b", 9, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=1585152",
    ("qwen2_7b", 64, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11272192",
    ("qwen2_7b", 65, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11448320",
    ("qwen2_7b", 128, "bf16", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=22544384",
    ("qwen2_7b", 129, "bf16", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=34080768",
    ("qwen2_7b", 255, "bf16", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67368960",
    ("qwen2_7b", 256, "bf16", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67633152",
    ("qwen2_7b", 257, "bf16", True): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    ("qwen2_7b", 1, "bf16", False): "4/1r 4/1r 4/1r 4/1r lm=4 ws=0",
    ("qwen2_7b", 8, "bf16", False): "4/1r 4/1r 4/1r 4/1r lm=4 ws=0",
    ("qwen2_7b", 9, "bf16", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=1585152",
    ("qwen2_7b", 64, "bf16", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=11272192",
    ("qwen2_7b", 65, "bf16", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=5724160",
    ("qwen2_7b", 128, "bf16", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=11272192",
    ("qwen2_7b", 129, "bf16", False): "2/1r 2/3r 2/1r 2/3r lm=0 ws=8520192",
    ("qwen2_7b", 255, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11228160",
    ("qwen2_7b", 256, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11272192",
    ("qwen2_7b", 257, "bf16", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    ("qwen2_7b", 1, "fp8", True): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("qwen2_7b", 8, "fp8", True): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("qwen2_7b", 9, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=1585152",
    ("qwen2_7b", 64, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11272192",
    ("qwen2_7b", 65, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=11448320",
    ("qwen2_7b", 128, "fp8", True): "5/2p 5/8p 5/1p 5/8p lm=0 ws=22544384",
    ("qwen2_7b", 129, "fp8", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=34080768",
    ("qwen2_7b", 255, "fp8", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67368960",
    ("qwen2_7b", 256, "fp8", True): "3/4r 3/8r 3/2r 3/12r lm=0 ws=67633152",
    ("qwen2_7b", 257, "fp8", True): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
    ("qwen2_7b", 1, "fp8", False): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("qwen2_7b", 8, "fp8", False): "fp8w/1f fp8w/1f fp8w/1f fp8w/1f lm=4 ws=0",
    ("qwen2_7b", 9, "fp8", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=1585152",
    ("qwen2_7b", 64, "fp8", False): "2/3r 2/8r 2/2r 2/8r lm=0 ws=11272192",
    ("qwen2_7b", 65, "fp8", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=5724160",
    ("qwen2_7b", 128, "fp8", False): "2/2r 2/4r 2/1r 2/4r lm=0 ws=11272192",
    ("qwen2_7b", 129, "fp8", False): "2/1r 2/3r 2/1r 2/3r lm=0 ws=8520192",
    ("qwen2_7b", 255, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11228160",
    ("qwen2_7b", 256, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11272192",
    ("qwen2_7b", 257, "fp8", False): "2/1r 2/2r 2/1r 2/2r lm=0 ws=11316224",
}


@pytest.mark.parametrize("model,Bn,wd,dp", CASES)
def test_plan_table_is_pinned(model, Bn, wd, dp):
    plan = _plan(model, Bn, wd, dp)
    got = " ".join(f"{g.tile}/{g.split_k}{g.weight[0]}" for g in (plan.sites[k] for k in E.DECODE_SITES))
    got += f" lm={plan.sites['lm_head'].tile} ws={plan.workspace}"
    assert got == PINNED[(model, Bn, wd, dp)]


def test_pinned_table_covers_every_case():
    assert set(PINNED) == set(CASES)


@pytest.mark.parametrize("Bn", (129, 200, 256))
def test_decode_t256_override_keeps_sites_on_the_decode_tile(Bn):
    """ICL_DECODE_T256 lists the sites that may move to the 256x256 tile above 128 rows; the others stay on tile 5."""
    for model in MODELS:
        full = _plan(model, Bn, "bf16", True)
        only_o = _plan(model, Bn, "bf16", True, decode_t256=("o",))
        none = _plan(model, Bn, "bf16", True, decode_t256=())
        for name in E.DECODE_SITES:
            assert none.sites[name].tile == 5 and none.sites[name].weight == "packed"
            assert only_o.sites[name] == (full.sites[name] if name == "o" else none.sites[name])


def test_unfused_norms():
    plan = _plan("llama2_7b", 64, "bf16", True, fuse_norms=False)
    assert not any(g.fused_norm for g in plan.sites.values())


def test_runtime_plans_with_its_own_settings():
    """LlamaHIP.decode_plan forwards the runtime's CU count, weight mode and class-level switches (no GPU needed)."""
    class W:
        cfg = MODELS["llama2_7b"]
        k_aug = llama_k_aug(cfg)
    rt = object.__new__(E.LlamaHIP)
    rt.w, rt.n_cu, rt.weight_dtype = W, N_CU, "fp8"
    for Bn in BATCHES:
        assert rt.decode_plan(Bn) == _plan("llama2_7b", Bn, "fp8", True)
    rt.decode_packed_weights, rt.fuse_decode_norms, rt.decode_t256 = False, False, ()
    assert rt.decode_plan(64) == _plan("llama2_7b", 64, "fp8", False, fuse_norms=False, decode_t256=())


# The same planner on a 304-CU device (MI300X), bf16 weights: where the CU count, not K, bounds the split, so the K-depth limits
# (sk5 / the 64x64 tile's K // 512, the latter's cap of 16 slices) decide some splits.
PINNED_304 = {
    ("llama2_7b", 1, True): "6/1p 6/1p 6/1p 6/1p",
    ("llama2_7b", 8, True): "6/1p 6/1p 6/1p 6/1p",
    ("llama2_7b", 9, True): "5/3p 5/8p 5/1p 5/9p",
    ("llama2_7b", 64, True): "5/3p 5/8p 5/1p 5/9p",
    ("llama2_7b", 65, True): "5/3p 5/8p 5/1p 5/9p",
    ("llama2_7b", 128, True): "5/3p 5/8p 5/1p 5/9p",
    ("llama2_7b", 129, True): "3/5r 5/8p 3/2r 3/15r",
    ("llama2_7b", 255, True): "3/5r 5/8p 3/2r 3/15r",
    ("llama2_7b", 256, True): "3/5r 5/8p 3/2r 3/15r",
    ("llama2_7b", 257, True): "2/1r 2/2r 2/1r 2/2r",
    ("llama2_7b", 1, False): "4/1r 4/1r 4/1r 4/1r",
    ("llama2_7b", 8, False): "4/1r 4/1r 4/1r 4/1r",
    ("llama2_7b", 9, False): "2/4r 2/8r 2/2r 2/10r",
    ("llama2_7b", 64, False): "2/4r 2/8r 2/2r 2/10r",
    ("llama2_7b", 65, False): "2/2r 2/5r 2/1r 2/5r",
    ("llama2_7b", 128, False): "2/2r 2/5r 2/1r 2/5r",
    ("llama2_7b", 129, False): "2/2r 2/4r 2/1r 2/4r",
    ("llama2_7b", 255, False): "2/1r 2/3r 2/1r 2/3r",
    ("llama2_7b", 256, False): "2/1r 2/3r 2/1r 2/3r",
    ("llama2_7b", 257, False): "2/1r 2/2r 2/1r 2/2r",
    ("llama2_13b", 1, True): "6/1p 6/1p 6/1p 6/1p",
    ("llama2_13b", 8, True): "6/1p 6/1p 6/1p 6/1p",
    ("llama2_13b", 9, True): "5/2p 5/7p 5/1p 5/7p",
    ("llama2_13b", 64, True): "5/2p 5/7p 5/1p 5/7p",
    ("llama2_13b", 65, True): "5/2p 5/7p 5/1p 5/7p",
    ("llama2_13b", 128, True): "5/2p 5/7p 5/1p 5/7p",
    ("llama2_13b", 129, True): "3/4r 3/10r 3/2r 3/12r",
    ("llama2_13b", 255, True): "3/4r 3/10r 3/2r 3/12r",
    ("llama2_13b", 256, True): "3/4r 3/10r 3/2r 3/12r",
    ("llama2_13b", 257, True): "2/1r 2/2r 2/1r 2/2r",
    ("llama2_13b", 1, False): "4/1r 4/1r 4/1r 4/1r",
    ("llama2_13b", 8, False): "4/1r 4/1r 4/1r 4/1r",
    ("llama2_13b", 9, False): "2/3r 2/8r 2/2r 2/8r",
    ("llama2_13b", 64, False): "2/3r 2/8r 2/2r 2/8r",
    ("llama2_13b", 65, False): "2/2r 2/4r 2/1r 2/4r",
    ("llama2_13b", 128, False): "2/2r 2/4r 2/1r 2/4r",
    ("llama2_13b", 129, False): "2/1r 2/3r 2/1r 2/3r",
    ("llama2_13b", 255, False): "2/1r 2/2r 2/1r 2/2r",
    ("llama2_13b", 256, False): "2/1r 2/2r 2/1r 2/2r",
    ("llama2_13b", 257, False): "2/1r 2/2r 2/1r 2/2r",
    ("qwen2_7b", 1, True): "6/1p 6/1p 6/1p 6/1p",
    ("qwen2_7b", 8, True): "6/1p 6/1p 6/1p 6/1p",
    ("qwen2_7b", 9, True): "5/3p 5/8p 5/1p 5/9p",
    ("qwen2_7b", 64, True): "5/3p 5/8p 5/1p 5/9p",
    ("qwen2_7b", 65, True): "5/3p 5/8p 5/1p 5/9p",
    ("qwen2_7b", 128, True): "5/3p 5/8p 5/1p 5/9p",
    ("qwen2_7b", 129, True): "3/5r 5/8p 3/2r 3/15r",
    ("qwen2_7b", 255, True): "3/5r 5/8p 3/2r 3/15r",
    ("qwen2_7b", 256, True): "3/5r 5/8p 3/2r 3/15r",
    ("qwen2_7b", 257, True): "2/1r 2/2r 2/1r 2/2r",
    ("qwen2_7b", 1, False): "4/1r 4/1r 4/1r 4/1r",
    ("qwen2_7b", 8, False): "4/1r 4/1r 4/1r 4/1r",
    ("qwen2_7b", 9, False): "2/4r 2/8r 2/2r 2/10r",
    ("qwen2_7b", 64, False): "2/4r 2/8r 2/2r 2/10r",
    ("qwen2_7b", 65, False): "2/2r 2/5r 2/1r 2/5r",
    ("qwen2_7b", 128, False): "2/2r 2/5r 2/1r 2/5r",
    ("qwen2_7b", 129, False): "2/2r 2/4r 2/1r 2/4r",
    ("qwen2_7b", 255, False): "2/1r 2/3r 2/1r 2/3r",
    ("qwen2_7b", 256, False): "2/1r 2/3r 2/1r 2/3r",
    ("qwen2_7b", 257, False): "2/1r 2/2r 2/1r 2/2r",
}


@pytest.mark.parametrize("model,Bn,dp", sorted(PINNED_304))
def test_plan_table_is_pinned_at_304_cus(model, Bn, dp):
    cfg = MODELS[model]
    plan = E.decode_plan(Bn, cfg, llama_k_aug(cfg), 304, "bf16", dp)
    assert " ".join(f"{g.tile}/{g.split_k}{g.weight[0]}" for g in (plan.sites[k] for k in E.DECODE_SITES)) == PINNED_304[(model, Bn, dp)]


@pytest.mark.parametrize("N,K,n_cu,want", [
    (4096, 4096, 256, 8),      # o at 7B: 16 N-tiles x 8 slices (K // 512)
    (4096, 4096, 270, 8),      # 128 blocks >= 0.45 * 270 = 121.5
    (4096, 4096, 285, 0),      # 128 blocks < 0.45 * 285 = 128.25: stays on the decode tile
    (22016, 4096, 256, 2),     # gu at 7B: 86 N-tiles, 204 // 86 = 2 slices
    (22016, 4096, 200, 0),     # 160 // 86 = 1 slice: < 2, no split worth the reduction
    (16384, 1024, 256, 2),     # 64 N-tiles: K // 512 = 2 (not 204 // 64 = 3) keeps every slice >= 8 K-tiles deep
    (16384, 512, 256, 0),      # K // 512 = 1
    (12288, 4160, 256, 4),     # qkv at 7B: 48 N-tiles, min(8, 204 // 48 = 4)
])
def test_t256_split_rules(N, K, n_cu, want):
    """t256_split: <= 0.8 * n_cu slices in all, >= 8 K-tiles per slice, >= 2 slices, >= 0.45 * n_cu blocks, else 0."""
    assert E.t256_split(N, K, n_cu) == want
