"""The 64x64 / 128x128 / 256x256 tiles of icl_gemm_bf16 (tiles 2 / 1 / 3) as the encoders and the LLM prefill launch them, every
output element against a float64 reference with the per-element bounds of tests/fp64_bounds.py (`-m gpu`).

Every output starts as NaN (an element the grid misses fails) and lies inside a larger allocation — guard rows above and below,
pad columns to the right — filled with a sentinel that must survive.  Activations are randn * 0.5, weights randn * 0.075, bias
and residual O(1): a dropped bias or residual is hundreds of bounds wide.

Groups: (a) epilogue x store-path matrix of the 256x256 tile, (b) the same epilogues on the other two tiles, (c) the
bit-identity contracts the tile chooser and batch invariance rest on, (d) the XCD-synchronised block -> tile map, (e) the
encoders' strided / batched launch forms and the column-section forms of the fused RoPE GEMM.  The worst err / bound ratio
of each group is printed when the module finishes (`-s`)."""
import pytest
import torch

import fp64_bounds as fb
from gpu_support import DEV, B, stop_after_a_device_fault  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENT = 7.0
GUARD_TOP, GUARD_BOT = 8, 3
EPIS = ("plain", "gelu", "res", "gelu_res", "swiglu")
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for grp in sorted(RATIOS):
        print(f"\nworst err/bound, group {grp}: {RATIOS[grp]:.4f}")


def _note(grp, got, ref, bound):
    RATIOS[grp] = max(RATIOS.get(grp, 0.0), fb.worst_ratio(got, ref, bound))


def _randn(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


_PROBLEMS = {}


def _problem(M, N, K):
    """a [M, K], w [N, K] (bf16) and their float64 product and magnitude: computed once per shape, never written to."""
    key = (M, N, K)
    if key not in _PROBLEMS:
        if len(_PROBLEMS) > 24:
            _PROBLEMS.clear()
        a = _randn((M, K), 1000 + M + K, 0.5, torch.bfloat16)
        w = _randn((N, K), 2000 + N + K, 0.075, torch.bfloat16)
        _PROBLEMS[key] = (a, w) + fb.dot64(a, w)
    return _PROBLEMS[key]


def _share_rows(M_big, M, N, K):
    """Register the first M rows of the M_big x N x K problem as the M x N x K problem (same activations, same weights)."""
    a, w, dot, mag = _problem(M_big, N, K)
    _PROBLEMS[(M, N, K)] = (a[:M], w, dot[:M], mag[:M])


def _guarded(M, ncols, ld, dtype, fill=float("nan")):
    """(buf, view): view = M x ncols of `fill` at row GUARD_TOP of a sentinel buffer [GUARD_TOP + M + GUARD_BOT, ld]."""
    buf = torch.full((GUARD_TOP + M + GUARD_BOT, ld), SENT, dtype=dtype, device=DEV)
    view = buf[GUARD_TOP:GUARD_TOP + M, :ncols]
    view.fill_(fill)
    return buf, view


def _assert_guard(buf, view, what):
    chk = buf.clone()
    chk[GUARD_TOP:GUARD_TOP + view.shape[0], :view.shape[1]] = SENT
    assert bool((chk == SENT).all()), f"{what}: wrote outside its M x N output"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(B, grp, M, N, K, *, tile, out_dtype, epi, with_bias, res="f32", variant="staged", res_rows=None):
    """One launch of the M x N x K problem, checked per element.  variant: the layout of C / bias (see the group-a test);
    res: "f32" | "bf16" | "inplace" (the f32 residual stream: out is residual); res_rows: draw the residual for this many rows
    and use the first M (two launches that share rows).  Returns the output view."""
    a, w, dot, mag = _problem(M, N, K)
    swiglu, gelu, has_res = epi == "swiglu", "gelu" in epi, "res" in epi
    nout = N // 2 if swiglu else N
    ld = {"staged": nout + 8, "direct": nout + 4, "scalar_n": nout + 1, "scalar_bias": nout + 8}[variant]
    bias = None
    if with_bias:
        store = _randn((N + 8,), 31)
        bias = store[1:1 + N] if variant == "scalar_bias" else store[4:4 + N]
    r = None
    if has_res:
        r = _randn((res_rows or M, ld), 32)[:M, :nout]
        if res == "bf16":
            r = r.to(torch.bfloat16)
    buf, out = _guarded(M, nout, ld, out_dtype)
    if has_res and res == "inplace":
        out.copy_(r)
        B.gemm(a, w, out, bias=bias, gelu=gelu, residual=out, tile=tile)
    else:
        B.gemm(a, w, out, bias=bias, gelu=gelu, swiglu=swiglu, residual=r, tile=tile)
    torch.cuda.synchronize()
    if swiglu:
        ref, e = fb.swiglu_ref_bound(dot, mag, K, bias=bias)
    else:
        ref, e = fb.gemm_ref_bound(dot, mag, K, bias=bias, residual=r, gelu=gelu)
    if out_dtype == torch.bfloat16:
        e = fb.bf16_out_bound(e, ref, out)
    what = f"tile {tile} {M}x{N}x{K} {epi} {'bias ' if with_bias else ''}{str(out_dtype)[6:]} out, {res} res, {variant}"
    fb.assert_within(out, ref, e, what)
    _assert_guard(buf, out, what)
    _note(grp, out, ref, e)
    return out


def _cases_a():
    out = []
    for od in (torch.bfloat16, torch.float32):
        for epi in EPIS:
            for wb in (False, True):
                for variant in ("staged", "direct", "scalar_n", "scalar_bias"):
                    if variant == "scalar_bias" and not wb:
                        continue
                    if variant == "scalar_n" and epi == "swiglu":
                        continue          # SwiGLU needs N % 32 == 0 and ldc % 4 == 0: its scalar form is the bias pointer's
                    if variant == "direct" and od == torch.float32 and "res" not in epi:
                        continue          # an f32 C with ldc % 4 == 0 is always whole 16-B rows: only a bf16 residual gets there
                    out.append(pytest.param(od, epi, wb, variant, id=f"{str(od)[6:]}-{epi}-{'bias' if wb else 'nobias'}-{variant}"))
    return out


# ---- a. epilogue x store-path matrix of the 256x256 tile --------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype,epi,with_bias,variant", _cases_a())
def test_tile3_epilogues_on_every_store_path(B, out_dtype, epi, with_bias, variant):
    """M = 300, N = 520 (SwiGLU: 544 interleaved columns) is 2 x 3 tiles of 256: two interior tiles, the M edge, the N edge
    and the corner; K = 128, 192, 256, 320 are nk = 2 (no steady K-tile), n_steady = 1 (odd), 2 (even) and 3 (odd after one
    unrolled pair): the three tails that pick the run-time buffer offset in gemm256.hip.  The ten instantiations are
    out {bf16, f32} x {plain, GELU, residual, GELU + residual, SwiGLU}; the bias is a run-time flag of each.

    variant (which predicate of gemm256_bf16_kernel it is meant to flip, for the interior tiles):
      staged       ldc = N + 8, every pointer 16-B aligned: vec_path_ok, rows16 (and res_rows for an f32 residual into an f32
                   C, also in place: out is residual) -> the LDS-staged row stores.  A bf16 residual, or an f32 residual into a
                   bf16 C, has res_rows false -> direct fragments.
      direct       bf16 C with ldc = N + 4: rows16 false (ldc * 2 % 16 = 8); f32 C with a bf16 residual: res_rows false ->
                   `else if (interior)`, direct 4-column fragments, the bias folded into the accumulators.
      scalar_n     N = 518, ldc = ldr = 519: vec_path_ok false (N % 4, ldc % 4) -> no interior tile, no folded bias; every
                   tile takes epi_store4's scalar loop with the bias added after the K loop.
      scalar_bias  N = 520, ldc = N + 8, but the bias pointer is 4 B past a 16-B boundary: vec_path_ok false through its last
                   clause -> the bounds-checked path with vector stores (vec_ok of epi_store4) and the bias added after."""
    N = 544 if epi == "swiglu" else (518 if variant == "scalar_n" else 520)
    kinds = ("f32",)
    if "res" in epi:
        kinds = ("f32", "bf16") + (("inplace",) if out_dtype == torch.float32 and variant == "staged" else ())
        if variant == "direct" and out_dtype == torch.float32:
            kinds = ("bf16",)
    for K in (128, 192, 256, 320):
        for res in kinds:
            _run(B, "a", 300, N, K, tile=3, out_dtype=out_dtype, epi=epi, with_bias=with_bias, res=res, variant=variant)


# ---- b. the same epilogues on the 128x128 and 64x64 tiles ------------------------------------------------------------------------
@pytest.mark.parametrize("tile,M,N,epi,variant", [
    (t, m, n, e, v) for t, m, n in ((1, 150, 200), (2, 70, 136)) for e in EPIS for v in ("staged", "scalar_n", "scalar_bias")
    if not (e == "swiglu" and v == "scalar_n")])      # SwiGLU needs N % 32 == 0 and ldc % 4 == 0: that launch does not exist
def test_tiles_1_and_2_epilogues(B, tile, M, N, epi, variant):
    """Tile 1 at 150 x 200 and tile 2 at 70 x 136, K = 192 (2 x 2 and 2 x 3 tiles: one interior tile, both edges, the corner),
    both output types, with and without bias, f32 and bf16 residual; `staged` is these tiles' vector path (folded bias,
    16-B fragments), the other two their scalar / unfolded forms as in group a."""
    if epi == "swiglu":
        N = {200: 224, 136: 160}[N]
    elif variant == "scalar_n":
        N -= 2
    for od in (torch.bfloat16, torch.float32):
        for wb in ((True,) if variant == "scalar_bias" else (False, True)):
            for res in (("f32", "bf16") if "res" in epi else ("f32",)):
                _run(B, "b", M, N, 192, tile=tile, out_dtype=od, epi=epi, with_bias=wb, res=res, variant=variant)


@pytest.mark.parametrize("epi", EPIS)
def test_tile3_below_k128_is_the_tile1_launch(B, epi):
    """K = 64 cannot feed the 256x256 pipeline's two peeled K-tiles: the host sends tile 3 to tile 1, bit for bit."""
    N = 224 if epi == "swiglu" else 200
    for od in (torch.bfloat16, torch.float32):
        o3 = _run(B, "b", 150, N, 64, tile=3, out_dtype=od, epi=epi, with_bias=True)
        o1 = _run(B, "b", 150, N, 64, tile=1, out_dtype=od, epi=epi, with_bias=True)
        assert torch.equal(_bits(o3), _bits(o1))


# ---- c. bit-identity contracts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", EPIS)
def test_tiles_1_2_3_give_the_same_bits(B, epi):
    """gemm.hip: "Tiles 1 - 3 sum K in the same order, so the choice never changes a row's bits" — icl_gemm_select_tile
    depends on M, so batch invariance rests on it.  Compared as integers (-0.0 != +0.0); M = 300, N = 520, K = 320, no split."""
    N = 544 if epi == "swiglu" else 520
    for od in (torch.float32, torch.bfloat16):
        for wb in (True, False):
            outs = [_run(B, "c", 300, N, 320, tile=t, out_dtype=od, epi=epi, with_bias=wb) for t in (1, 2, 3)]
            assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"tiles 1 and 2 differ ({epi}, {od}, bias {wb})"
            assert torch.equal(_bits(outs[0]), _bits(outs[2])), f"tiles 1 and 3 differ ({epi}, {od}, bias {wb})"


@pytest.mark.parametrize("epi", EPIS)
def test_rows_do_not_depend_on_the_launch_height(B, epi):
    """The rows of an M = 300 launch == the same rows inside an M = 1100 launch, the library choosing the tile for both
    (tile 0), and both inside the float64 bound."""
    N, K = (544 if epi == "swiglu" else 520), 320
    _share_rows(1100, 300, N, K)
    for od in (torch.float32, torch.bfloat16):
        big = _run(B, "c", 1100, N, K, tile=0, out_dtype=od, epi=epi, with_bias=True, res_rows=1100)
        small = _run(B, "c", 300, N, K, tile=0, out_dtype=od, epi=epi, with_bias=True, res_rows=1100)
        assert torch.equal(_bits(small), _bits(big[:300]))
    del _PROBLEMS[(300, N, K)]


@pytest.mark.parametrize("tile,bm", [(1, 128), (2, 64)])
def test_deep_ring_and_two_stage_forms_give_the_same_bits(B, tile, bm):
    """launch_tile (gemm.hip) takes the deep LDS ring (TILE_STAGES_DEEP: 3 K-tiles on the 128x128 tile, 4 on the 64x64 one)
    when all blocks fit on the chip at its footprint, blocks <= n_cu * (160 KiB / ring bytes), and the two-stage form
    otherwise: "The choice does not change a bit of the result."  300 x 2000 is under the limit, 2100 x 2000 over it; K = 128."""
    n_cu = B.device_cu_count()
    deep = 4 if 2 * bm <= 128 else 3
    per_cu = (160 * 1024) // (2 * bm * 128 * deep)
    blocks = lambda m: -(-m // bm) * -(-2000 // bm)     # noqa: E731
    assert blocks(300) <= n_cu * per_cu < blocks(2100), (n_cu, per_cu, blocks(300), blocks(2100))
    _share_rows(2100, 300, 2000, 128)
    for od in (torch.float32, torch.bfloat16):
        big = _run(B, "c", 2100, 2000, 128, tile=tile, out_dtype=od, epi="gelu", with_bias=True)
        small = _run(B, "c", 300, 2000, 128, tile=tile, out_dtype=od, epi="gelu", with_bias=True)
        assert torch.equal(_bits(small), _bits(big[:300]))
    del _PROBLEMS[(300, 2000, 128)]


# ---- d. the XCD-synchronised block -> tile map ------------------------------------------------------------------------------------
def _tile_map(M, N, K):
    """(gm, tiles_m, tiles_n, covered) of launch_tile256 / block_to_tile for this shape."""
    tiles_m, tiles_n = -(-M // 256), -(-N // 256)
    gm = min(6, max(1, 8400000 // (512 * K)))
    return gm, tiles_m, tiles_n, ((tiles_m // gm) >> 3) * 8 * gm * tiles_n


@pytest.mark.parametrize("M,N,K,want", [(2104, 300, 8256, (1, 9, 2, 16)), (4764, 520, 5504, (2, 19, 3, 48)),
                                        (1800, 520, 1280, (6, 8, 3, 0))])
def test_tile3_xcd_synchronised_tile_map(B, M, N, K, want):
    """block_to_tile (gemm_common.h) deals the first `covered` blocks to super-tiles x, x + 8, ... per XCD and the rest by the
    contiguous split.  2104 x 300 x 8256: gm = 1, 9 M-tiles, 8 covered + a one-tile tail.  4764 x 520 x 5504: gm = 2, 19
    M-tiles, 16 covered, then a full super-tile and a ragged one, with M and N edges.  1800 x 520 x 1280 is the control:
    gm = 6, 8 M-tiles, nothing covered, a ragged second super-tile.  A tile the map misses stays NaN, one it deals twice is
    harmless, so with a bijection of blocks onto tiles every element is written.  gm and covered are recomputed here from the
    heuristic of launch_tile256: a change of it that empties the branch fails this test instead of un-testing the branch."""
    gm, tiles_m, tiles_n, covered = _tile_map(M, N, K)
    print(f"\n{M}x{N}x{K}: gm {gm} tiles_m {tiles_m} tiles_n {tiles_n} covered {covered} of {tiles_m * tiles_n}")
    assert (gm, tiles_m, tiles_n, covered) == want
    assert (covered > 0) == (want[3] > 0) and covered < tiles_m * tiles_n
    _run(B, "d", M, N, K, tile=3, out_dtype=torch.float32, epi="res", with_bias=True, res="f32", variant="staged")
    _PROBLEMS.pop((M, N, K), None)


# ---- e. the encoders' launch forms ------------------------------------------------------------------------------------------------
def _batched_guard(n_items, rows, cols, dtype, fill):
    """[n_items + 2, rows, cols] sentinel buffer whose items 1 .. n_items hold `fill`."""
    buf = torch.full((n_items + 2, rows, cols), SENT, dtype=dtype, device=DEV)
    buf[1:1 + n_items] = fill
    return buf, buf[1:1 + n_items]


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
def test_whisper_conv1_form(B, tile):
    """conv1 (k = 3, p = 1) as a GEMM over overlapping rows: row t of an item is xt[t : t + 3, :128] (lda = 128 < K = 384),
    3 items, bias + GELU, written into rows 1 .. 300 of a zeroed [3, 302, 320] bf16 tensor (stride_c = 302 * 320): rows 0 and
    301 of every item are conv2's zero padding and must still be zero."""
    n, T, d = 3, 300, 320
    xt = _randn((n, T + 2, 128), 41, 0.5, torch.bfloat16)
    w = _randn((d, 384), 42, 0.075, torch.bfloat16)
    bias = _randn((d,), 43)
    buf, x2 = _batched_guard(n, T + 2, d, torch.bfloat16, 0.0)
    x2[:, 1:T + 1] = float("nan")
    B.gemm(xt, w, x2[:, 1:], bias=bias, gelu=True, M=T, K=384, lda=128, batch=n, stride_a=(T + 2) * 128, stride_c=(T + 2) * d,
           tile=tile)
    torch.cuda.synchronize()
    a = torch.cat([xt[:, j:j + T] for j in range(3)], -1)              # [n, T, 384]
    dot, mag = fb.dot64(a, w)
    ref, e = fb.gemm_ref_bound(dot, mag, 384, bias=bias, gelu=True)
    got = x2[:, 1:T + 1]
    e = fb.bf16_out_bound(e, ref, got)
    fb.assert_within(got.reshape(n * T, d), ref.reshape(n * T, d), e.reshape(n * T, d), f"conv1 form, tile {tile}")
    assert bool((x2[:, 0] == 0).all()) and bool((x2[:, T + 1] == 0).all()), "conv1 wrote a padding row"
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    _note("e", got, ref, e)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
def test_whisper_conv2_form(B, tile):
    """conv2 (k = 3, s = 2, p = 1): row t of an item is x2[2t : 2t + 3, :] (lda = 2d, K = 3d, d = 320), 3 items of 150 rows,
    bias + GELU, then the SAME [150, 320] f32 table added to every item (stride_r = 0), after the GELU."""
    n, T, d = 3, 150, 320
    x2 = _randn((n, 2 * T + 2, d), 44, 0.5, torch.bfloat16)
    w = _randn((d, 3 * d), 45, 0.075, torch.bfloat16)
    bias, pos = _randn((d,), 46), _randn((T, d), 47)
    buf, h = _batched_guard(n, T, d, torch.float32, float("nan"))
    B.gemm(x2, w, h, bias=bias, gelu=True, residual=pos, M=T, K=3 * d, lda=2 * d, batch=n, stride_a=(2 * T + 2) * d,
           stride_c=T * d, stride_r=0, tile=tile)
    torch.cuda.synchronize()
    a = torch.cat([x2[:, j:j + 2 * T:2][:, :T] for j in range(3)], -1)  # [n, T, 3d]
    dot, mag = fb.dot64(a, w)
    ref, e = fb.gemm_ref_bound(dot, mag, 3 * d, bias=bias, residual=pos, gelu=True)
    fb.assert_within(h.reshape(n * T, d), ref.reshape(n * T, d), e.reshape(n * T, d), f"conv2 form, tile {tile}")
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    _note("e", h, ref, e)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("g", [0, 7, 15])
def test_beats_posconv_form(B, g, tile):
    """The BEATs grouped positional conv, group g of 16: N = 48 output channels, K = 128 taps x 48 channels over the group's
    padded [T + 128, 48] image (lda = 48: row t starts 48 elements after row t - 1), T = 72, 2 items; C and R are the 48-column
    slices g of [144, 768] f32 tensors; bias + GELU + residual.  The other 720 columns keep their sentinel, and the ragged
    form of the call (one launch per item, batch 1) gives the same bits."""
    n, T, d, cpg = 2, 72, 768, 48
    K = 128 * cpg
    xg = _randn((n * (T + 128) * d,), 51, 0.5, torch.bfloat16)
    w = _randn((cpg, K), 52 + g, 0.05, torch.bfloat16)
    bias_all, x = _randn((d,), 53), _randn((n * T, d), 54)
    bg = bias_all[g * cpg:(g + 1) * cpg]

    def fresh():
        y = torch.full((n * T + 2, d), SENT, device=DEV)
        y[1:1 + n * T, g * cpg:(g + 1) * cpg] = float("nan")
        return y, y[1:1 + n * T]
    ybuf, y = fresh()
    B.gemm(xg[g * (T + 128) * cpg:], w, y[:, g * cpg:], bias=bg, gelu=True, residual=x[:, g * cpg:], M=T, K=K, lda=cpg, batch=n,
           stride_a=(T + 128) * d, stride_c=T * d, stride_r=T * d, tile=tile)
    zbuf, z = fresh()
    for it in range(n):
        base = (it * T + 128 * it) * d + g * (T + 128) * cpg
        B.gemm(xg[base:], w, z[it * T:(it + 1) * T, g * cpg:], bias=bg, gelu=True, residual=x[it * T:(it + 1) * T, g * cpg:], M=T,
               K=K, lda=cpg, tile=tile)
    torch.cuda.synchronize()
    img = xg.view(n, d * (T + 128))[:, g * (T + 128) * cpg:(g + 1) * (T + 128) * cpg].reshape(n, T + 128, cpg)
    a = img.unfold(1, 128, 1).permute(0, 1, 3, 2)[:, :T].reshape(n * T, K)
    dot, mag = fb.dot64(a, w)
    ref, e = fb.gemm_ref_bound(dot, mag, K, bias=bg, residual=x[:, g * cpg:(g + 1) * cpg], gelu=True)
    got = y[:, g * cpg:(g + 1) * cpg]
    fb.assert_within(got, ref, e, f"pos-conv form, group {g}, tile {tile}")
    for buf in (ybuf, zbuf):
        chk = buf.clone()
        chk[1:1 + n * T, g * cpg:(g + 1) * cpg] = SENT
        assert bool((chk == SENT).all()), "pos-conv wrote outside its 48 columns"
    assert torch.equal(_bits(got), _bits(z[:, g * cpg:(g + 1) * cpg])), "uniform and ragged forms differ"
    _note("e", got, ref, e)


@pytest.mark.parametrize("with_bias", [False, True])
def test_rope_gemm_column_section_forms(B, with_bias):
    """The two launches of LlamaHIP._last_layer_rows on the fused RoPE GEMM, each bit for bit against icl_gemm_bf16 +
    icl_rope_kv_bf16 on the same column blocks: the k | v rows of wqkv over all rows into the cache only (k_off = 0,
    kv_rows_to_c = 0: C is never written), and the q rows of wqkv over a few gathered rows, rotated at their own positions
    (k_off = v_off = N, no cache)."""
    H, D, K, M, max_len = 2, 128, 320, 300, 128
    hd = H * D
    x = _randn((M, K), 61, 0.5, torch.bfloat16)
    wqkv = _randn((3 * hd, K), 62, 0.075, torch.bfloat16)
    bqkv = _randn((3 * hd,), 63) if with_bias else None
    lens = [100, 73, 127]
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(DEV)
    sid = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(lens)]).to(DEV)
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    ang = torch.arange(max_len, device=DEV).float()[:, None] * inv[None, :]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()

    def caches():
        kc = torch.full((len(lens), H, max_len, D), SENT, dtype=torch.bfloat16, device=DEV)
        return kc, kc.clone()
    # the unfused pair on the k | v column blocks
    tmp = torch.zeros(M, 3 * hd, dtype=torch.bfloat16, device=DEV)
    kc0, vc0 = caches()
    B.gemm(x, wqkv[hd:], tmp[:, hd:], bias=bqkv[hd:] if with_bias else None, tile=3)
    B.rope_kv(tmp, hd, 2 * hd, cos, sin, pos, sid, kc0, vc0, H, D, max_len)
    # fused, cache only
    c = torch.full((M, 3 * hd), SENT, dtype=torch.bfloat16, device=DEV)
    kc1, vc1 = caches()
    B.gemm(x, wqkv[hd:], c, bias=bqkv[hd:] if with_bias else None, tile=3,
           rope=(0, hd, cos, sin, pos, sid, kc1, vc1, H, D, max_len, False))
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc1), _bits(kc0)) and torch.equal(_bits(vc1), _bits(vc0))
    assert bool((c == SENT).all()), "kv_rows_to_c = 0 wrote C"
    for s, n in enumerate(lens):
        assert bool((kc1[s, :, :n] != SENT).any(-1).all()) and bool((kc1[s, :, n:] == SENT).all())
    # the q rows on gathered rows
    idx = torch.tensor([99, 172, 299, 0, 150], device=DEV)
    xg, pg = x[idx].contiguous(), pos[idx].contiguous()
    qt = torch.zeros(len(idx), 3 * hd, dtype=torch.bfloat16, device=DEV)
    B.gemm(xg, wqkv[:hd], qt, bias=bqkv[:hd] if with_bias else None, tile=3)
    B.rope_kv(qt, hd, 2 * hd, cos, sin, pg, None, None, None, H, D, max_len)
    qbuf, q = _guarded(len(idx), hd, hd, torch.bfloat16)
    B.gemm(xg, wqkv[:hd], q, bias=bqkv[:hd] if with_bias else None, tile=3,
           rope=(hd, hd, cos, sin, pg, None, None, None, H, D, max_len))
    torch.cuda.synchronize()
    assert torch.equal(_bits(q), _bits(qt[:, :hd]))
    _assert_guard(qbuf, q, "q-only RoPE GEMM")
