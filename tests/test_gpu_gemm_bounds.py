"""The bf16 GEMM forward kernels (csrc/gemm.hip) on the GPU: every case asserts the route the launcher really takes (ops.gemm_route: kernel id and
the staged-epilogue flag), runs the kernel once, and holds it to the exact expectation or the per-element bound of tests/gemm_reference.py,
printing `gemm bound: route ... worst ...` (pytest -s)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_reference as gr
from walkgpt_amd import ops

S = ops.GEMM_STAGED
RES_MOD = 100                                         # the cross's row-modulo residual: the wrap falls inside a 64-row slab
# bias yes / no  x  ReLU / none  x  residual none / full / row modulo
EPILOGUES = list(itertools.product((True, False), (gr.ACT_NONE, gr.ACT_RELU), (None, 0, RES_MOD)))


def _cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _exact_cross(dev, tile, want, out_f32, shapes, epilogues=EPILOGUES):
    """Every shape x epilogue: route `want` (id | flag), one launch, torch.equal with the stated roundings."""
    n = 0
    for M, N, K in shapes:
        a, w, b, _ = gr.exact_inputs(M, N, K, seed=M + N + K)
        acc = gr.exact_acc(a, w)
        ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
        for has_b, act, res_mod in epilogues:
            r = None if res_mod is None else gr.exact_inputs(M, N, K, seed=N + 1, rrows=res_mod or M)[3]
            rdv = None if r is None else r.to(dev)
            kw = dict(residual=rdv, tile=tile, res_row_mod=res_mod or 0, out_f32=out_f32)
            got = ops.gemm_route(ad, wd, bd if has_b else None, **kw)
            assert got == want, "M=%d N=%d K=%d: route %d (staged %d), the case is written for %d (staged %d)" % (M, N, K, got & 63, got >> 6, want & 63, want >> 6)
            out = ops.linear(ad, wd, bd if has_b else None, act=act, **kw)
            exp = gr.exact_expected(a, w, b if has_b else None, r, res_mod or 0, act, bool(want & S), out_f32, acc=acc)
            bad = (out.cpu() != exp)
            assert not bool(bad.any()), "route %d M=%d N=%d K=%d bias %d act %d res %s: %d elements differ, first at %s" % (
                want & 63, M, N, K, has_b, act, res_mod, int(bad.sum()), bad.nonzero()[0].tolist())
            n += 1
    print("gemm bound: route %d staged %d f32 %d: %d exact launches over %s, worst 0 (bit-exact)" % (want & 63, want >> 6, out_f32, n, shapes))


SMALL_TILES = [(M, N, K) for M in (129, 144, 300) for N in (128, 272) for K in (64, 192)]
BIG_MN = [(M, N) for M in (257, 300, 520) for N in (256, 264, 520)]


@pytest.mark.parametrize("out_f32", [False, True])
def test_route_1_exact_both_epilogues(dev, out_f32):
    _exact_cross(dev, 1, 1 | (0 if out_f32 else S), out_f32, SMALL_TILES)


def test_route_11_exact(dev):
    _exact_cross(dev, 11, 11 | S, False, SMALL_TILES)


def test_route_12_exact(dev):
    """The tail kernel takes M % 128 in 1 .. 16 only (wg_tail_rows): 272 = 2 * 128 + 16 stands where the other 128-row routes have 300."""
    _exact_cross(dev, 12, 12 | S, False, [(M, N, K) for M in (129, 144, 272) for N in (128, 272) for K in (64, 192)])


@pytest.mark.parametrize("out_f32", [False, True])
def test_route_2_exact_both_epilogues(dev, out_f32):
    _exact_cross(dev, 2, 2 | (0 if out_f32 else S), out_f32, [(M, N, K) for M, N in BIG_MN for K in (64, 192)])


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 512, 1024, 4096])
@pytest.mark.parametrize("tile,out_f32", [(14, False), (14, True), (16, False)])
def test_routes_14_16_exact_over_the_slab_ring(dev, tile, out_f32, K):
    """Both parities of the slab count (the seamless and the odd-nk flow of 16) and the ring over up to 64 slabs."""
    _exact_cross(dev, tile, tile | (0 if out_f32 else S), out_f32, [(M, N, K) for M, N in BIG_MN])


@pytest.mark.parametrize("tile", [1, 2, 14])
def test_unstaged_bf16_epilogue_exact(dev, tile):
    """N % 8 != 0: a bf16 output through the unstaged epilogue, ONE rounding after the residual add."""
    _exact_cross(dev, tile, tile, False, [(300, 268, 192), (257, 516, 128)])


def test_route_3_exact(dev):
    """Calls that fail wg_mfma_ok (K % 64, N % 4, N < 16): the row-wave kernel."""
    for out_f32 in (False, True):
        _exact_cross(dev, 0, 3, out_f32, [(37, 36, 100), (13, 4, 256), (20, 30, 64), (9, 8, 128)])


@pytest.mark.parametrize("K", [128, 256, 2048, 2560])
def test_route_5_exact_row_major_and_tiled(dev, K):
    """The skinny kernel, narrow (4 waves) and wide (16 waves: K >= 2048, K % 512 == 0), W row-major (ops.linear) and in fragment order
    (ops.layernorm_linear without a LayerNorm)."""
    for out_f32 in (False, True):
        _exact_cross(dev, 5, 5, out_f32, [(M, 48, K) for M in (1, 15, 16, 17, 128)])
    for M in (1, 15, 16, 17, 128):
        a, w, b, _ = gr.exact_inputs(M, 48, K, seed=M + K)
        ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
        assert ops.gemm_route(ad, wd, bd, tile=5) == 5
        for act, out_f32 in itertools.product((gr.ACT_NONE, gr.ACT_RELU), (False, True)):
            out = ops.layernorm_linear(ad, None, None, 0.0, wd, bd, act=act, out_f32=out_f32, weight_tiled=ops.tile_weight(wd))
            assert torch.equal(out.cpu(), gr.exact_expected(a, w, b, None, 0, act, False, out_f32))
    print("gemm bound: route 5 K %d tiled W: worst 0 (bit-exact)" % K)


@pytest.mark.parametrize("tile,out_f32,M,N", [(1, False, 300, 272), (1, True, 300, 272), (11, False, 300, 272), (12, False, 272, 272), (2, False, 520, 264),
                                              (14, False, 520, 264), (14, True, 520, 264), (16, False, 520, 264)])
def test_random_data_every_activation_under_the_bound(dev, tile, out_f32, M, N):
    """Random operands through every activation, with bias and a row-modulo residual, at an odd slab count (K = 320), against float64."""
    K = 320
    a, w, b, r = gr.random_inputs(M, N, K, seed=tile + M, rrows=RES_MOD)
    ad, wd, bd, rdv = a.to(dev), w.to(dev), b.to(dev), r.to(dev)
    want = tile | (0 if out_f32 else S)
    for act in (gr.ACT_NONE, gr.ACT_GELU, gr.ACT_QUICK_GELU, gr.ACT_RELU):
        assert ops.gemm_route(ad, wd, bd, rdv, tile=tile, res_row_mod=RES_MOD, out_f32=out_f32) == want
        out = ops.linear(ad, wd, bd, act=act, residual=rdv, res_row_mod=RES_MOD, tile=tile, out_f32=out_f32)
        worst, share = gr.check(out, gr.reference(a, w, b, r, RES_MOD, act), K, act, not out_f32, out_f32, True)
        print("gemm bound: route %d staged %d f32 %d act %d: worst %.3f" % (tile, not out_f32, out_f32, act, worst))
        assert worst <= 1.0 and share == 0.0


# ---- residual modulo through the staged epilogue ---------------------------------------------------------------------------------------

RES_MODS = [1, 7, 63, 64, 100, 128, 257]


def _wrap_positions(M, res_mods):
    """Where the row index wraps (m % res_mod == 0, m > 0) inside the 64-row slabs: the set of m % 64."""
    return {m % 64 for rm in res_mods for m in range(rm, M, rm)}


@pytest.mark.parametrize("tile,M,N", [(11, 300, 272), (12, 272, 272), (14, 520, 264), (16, 520, 264)])
def test_residual_row_modulo_staged_exact(dev, tile, M, N):
    """wg_load_residual's three branches (no modulo is in the cross above): res_mod >= 64 with one wrap inside a 64-row slab -- in its middle
    (100, 257), on its first row (64, 128: no wrap inside) and on its last row (63 is below 64, so 127 stands in for that branch) --, and
    res_mod < 64 with the per-row modulo (1, 7, 63).  R and A are column slices of wider tensors."""
    K = 192
    mods = RES_MODS + [127]
    pos = _wrap_positions(M, [rm for rm in mods if rm >= 64])
    assert 0 in pos and 63 in pos and any(0 < p < 63 for p in pos)            # a wrap on a slab's first row, its last row, in its middle
    assert 63 in _wrap_positions(M, [63])
    g = torch.Generator().manual_seed(tile)
    a_full = torch.randint(-3, 4, (M, 3 * K), generator=g).to(torch.bfloat16)
    a = a_full[:, K:2 * K]
    _, w, b, _ = gr.exact_inputs(M, N, K, seed=tile + 1)
    acc = gr.exact_acc(a, w)
    ad, wd, bd = a_full.to(dev)[:, K:2 * K], w.to(dev), b.to(dev)
    for rm in mods:
        r_full = torch.randint(-8, 9, (rm, N + 24), generator=g).to(torch.bfloat16)
        r = r_full[:, 8:8 + N]
        rdv = r_full.to(dev)[:, 8:8 + N]
        assert rdv.stride(0) == N + 24 and rdv.stride(0) % 8 == 0 and rdv.data_ptr() % 16 == 0
        for act in (gr.ACT_NONE, gr.ACT_RELU):
            assert ops.gemm_route(ad, wd, bd, rdv, tile=tile, res_row_mod=rm) == tile | S
            out = ops.linear(ad, wd, bd, act=act, residual=rdv, res_row_mod=rm, tile=tile)
            exp = gr.exact_expected(a, w, b, r, rm, act, True, False, acc=acc)
            bad = out.cpu() != exp
            assert not bool(bad.any()), "route %d res_mod %d act %d: %d elements differ, first at %s" % (tile, rm, act, int(bad.sum()), bad.nonzero()[0].tolist())
    print("gemm bound: route %d staged 1 res_mod %s: worst 0 (bit-exact)" % (tile, mods))


# ---- several tiles per workgroup -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [64, 128, 192, 320])
@pytest.mark.parametrize("tile,rows_per_cu,extra,N", [(16, 256, 1, 256), (16, 128, 2, 512), (11, 256, 1, 128)])
def test_more_tiles_than_workgroups_exact(dev, tile, rows_per_cu, extra, N, K):
    """The persistent kernels' hand-over from tile to tile, at both parities of the slab count: 16 with CU + 1 tiles (N = 256) and with
    2 * ceil((CU + 2) / 2) > CU tiles (N = 512), 11 with 2 CU + 1 tiles and a ragged last one (its grid is two workgroups per CU)."""
    cu = _cu(dev)
    M = rows_per_cu * cu + (128 * extra if tile == 16 and N == 512 else (256 if tile == 16 else 44))
    bt = 256 if tile == 16 else 128
    tiles = -(-M // bt) * -(-N // bt)
    assert tiles > (cu if tile == 16 else 2 * cu)
    _exact_cross(dev, tile, tile | S, False, [(M, N, K)], [(True, gr.ACT_RELU, RES_MOD), (False, gr.ACT_NONE, None)])


@pytest.mark.parametrize("tile", [14, 16])
def test_tile_order_with_a_narrower_last_column_block_exact(dev, tile):
    """M = 300, N = 2048, K = 1024: 4 MiB of weights, 512 KiB panels -> column blocks of 3 tile columns, the last block 2 wide (wg_tile_of)."""
    _exact_cross(dev, tile, tile | S, False, [(300, 2048, 1024)], [(True, gr.ACT_NONE, 0)])


# ---- kernel 17: LayerNorm folded in ----------------------------------------------------------------------------------------------------

def _ln_call(dev, d, stats, M, N, K, act):
    L = ops._lib.lib()
    x, wg = d["x"].to(dev), d["wg"].to(dev)
    assert L.wg_gemm_ln_supported(M, N, K, K, K, N) == 1 and ops.gemm_route(x, wg, tile=16) == 16 | S
    cs, bf, st = d["colsum"].to(dev), d["bias_f32"].to(dev), stats.to(dev)
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    rc = L.wg_gemm_ln_bias_act_bf16(x.data_ptr(), K, wg.data_ptr(), K, bf.data_ptr(), cs.data_ptr(), st.data_ptr(), out.data_ptr(), N, M, N, K, act,
                                    ops._stream())
    ops._lib.check(rc, "wg_gemm_ln_bias_act_bf16")
    return out.cpu()


@pytest.mark.parametrize("M,K", [(4096, 64), (4096, 192), (4096, 256), (4099, 192)])
def test_kernel_17_exact_with_handed_in_statistics(dev, M, K):
    """rstd * (x Wg^T - mean * s) + b' on integer rows, integer Wg / colsum / b', one {small integer mean, power-of-two rstd} per row, varied across
    rows: exact in fp32, so a row-permuted statistics load or a wrong column-sum term fails."""
    N = 1024
    d = gr.ln_exact_inputs(M, N, K, seed=M + K)
    for act in (gr.ACT_NONE, gr.ACT_RELU):
        bad = _ln_call(dev, d, d["stats"], M, N, K, act) != gr.ln_exact_expected(d, act)
        assert not bool(bad.any()), "kernel 17 M=%d K=%d act %d: %d elements differ, first at %s" % (M, K, act, int(bad.sum()), bad.nonzero()[0].tolist())
    print("gemm bound: route 17 (16 staged 1, LayerNorm folded) M %d K %d: worst 0 (bit-exact)" % (M, K))


@pytest.mark.parametrize("M,K", [(4099, 256), (4096, 192)])
def test_kernel_17_random_under_the_bound(dev, M, K):
    N, eps = 1024, 1e-6
    d = gr.ln_random_inputs(M, N, K, seed=M + K)
    st = gr.stats_fp32(d["x"], eps)
    prod = gr.ln_products(d["x"], d["wg"])
    for act in (gr.ACT_NONE, gr.ACT_GELU, gr.ACT_QUICK_GELU):
        rd = gr.ln_reference(d["x"], d["wg"], d["colsum"], d["bias_f32"], st, act, products=prod)
        worst, share = gr.check(_ln_call(dev, d, st, M, N, K, act), rd, K, act, True, False, False, gr.LN_EPILOGUE_OPS)
        print("gemm bound: route 17 (16 staged 1, LayerNorm folded) M %d K %d act %d: worst %.3f" % (M, K, act, worst))
        assert worst <= 1.0 and share == 0.0


# ---- kernels 18 -> 17 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(8195, 512, 64), (8195, 512, 192)])
def test_kernel_18_exact_output_and_partial_sums(dev, M, N, K):
    """Integer data: the stored values are integers (even ones above 256), and their sums and sums of squares per 256-column plane stay below
    2^24, so the partial planes equal the integer sums bit for bit in any summation order.  Rows M .. mpad are not read."""
    a, w, b, r = gr.exact_inputs(M, N, K, seed=M + K, rrows=M)
    ad, wd, bd, rdv = a.to(dev), w.to(dev), b.to(dev), r.to(dev)
    assert ops.gemm_route(ad, wd, bd, rdv, tile=16) == 16 | S
    with ops.time_gemms() as rec:
        y = ops.linear(ad, wd, bd, residual=rdv, row_partials=True)
    assert [k for k, *_ in rec] == [18] and y.partials is not None
    exp = gr.exact_expected(a, w, b, r, 0, gr.ACT_NONE, True, False)
    assert torch.equal(y.x.cpu(), exp)
    part, mpad = y.partials, y.partials.shape[1]
    assert part.shape == (N // 256, mpad, 2) and mpad == (M + 255) // 256 * 256
    yt = exp.double().view(M, N // 256, 256)
    assert (yt * yt).sum(-1).max().item() < 2 ** 24 and yt.abs().sum(-1).max().item() < 2 ** 24
    got = part[:, :M].cpu().double()
    assert torch.equal(got[..., 0].t(), yt.sum(-1)) and torch.equal(got[..., 1].t(), (yt * yt).sum(-1))
    print("gemm bound: route 18 (16 staged 1, row partial sums) M %d N %d K %d: worst 0 (bit-exact)" % (M, N, K))


@pytest.mark.parametrize("M,D,N2", [(16500, 256, 256), (5700, 768, 768), (3400, 1280, 1280)])
def test_kernel_17_fed_by_18s_partial_sums_under_the_bound(dev, M, D, N2):
    """wg_gemm_lnp_bias_act_bf16 with 1, 3 and 5 planes of partial sums left by the producing GEMM, against the float64 folded reference with
    float64 statistics of the stored rows; rows carry a mean of several sigma (the one-pass variance term of the bound)."""
    eps, Kp = 1e-6, 64
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, Kp, generator=g).to(torch.bfloat16)
    w = (torch.randn(D, Kp, generator=g) / Kp ** 0.5).to(torch.bfloat16)
    r = (torch.randn(M, D, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + 3.0 * torch.randn(M, 1, generator=g)).to(torch.bfloat16)
    y = ops.linear(x.to(dev), w.to(dev), residual=r.to(dev), row_partials=True)
    assert y.partials is not None and y.partials.shape[0] == D // 256
    gamma = (1.0 + 0.3 * torch.randn(D, generator=g)).to(torch.bfloat16)
    beta = (0.2 * torch.randn(D, generator=g)).to(torch.bfloat16)
    w2 = (torch.randn(N2, D, generator=g) / D ** 0.5).to(torch.bfloat16)
    b2 = torch.randn(N2, generator=g).to(torch.bfloat16)
    fold = ops.fold_layernorm(gamma.to(dev), beta.to(dev), w2.to(dev), b2.to(dev))
    assert ops.gemm_route(y.x, fold["wg"], tile=16) == 16 | S
    yc, wg, cs, bf = y.x.cpu(), fold["wg"].cpu(), fold["colsum"].cpu(), fold["bias_f32"].cpu()
    st = gr.row_stats64(yc, eps)
    prod = gr.ln_products(yc, wg)
    for act in (gr.ACT_NONE, gr.ACT_GELU):
        with ops.time_gemms() as rec:
            got = ops.ln_linear(y, fold, eps, act=act)
        assert [k for k, *_ in rec] == [17]                              # one launch: the statistics come from the partial sums
        rd = gr.ln_reference(yc, wg, cs, bf, st, act, from_partials=(D // 256, eps), products=prod)
        worst, share = gr.check(got, rd, D, act, True, False, False, gr.LN_EPILOGUE_OPS)
        print("gemm bound: route 17 fed by 18 (%d planes) M %d N %d act %d: worst %.3f" % (D // 256, M, N2, act, worst))
        assert worst <= 1.0 and share == 0.0


# ---- the skinny kernel with LayerNorm in front -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 15, 16, 17, 128])
@pytest.mark.parametrize("K", [256, 2048])
def test_skinny_layernorm_variants_under_the_bound(dev, M, K):
    """All four LN x tiled instances, narrow (K = 256, 4 waves) and wide (K = 2048, 16 waves), against float64 LayerNorm -> bf16 rounding ->
    GEMM; an outlier channel as LLM hidden states have."""
    N, eps = 48, 1e-5
    g = torch.Generator().manual_seed(13 + M + K)
    x = (torch.randn(M, K, generator=g) * 2.0 + 0.7).to(torch.bfloat16)
    x[:, 3] += 40.0
    gam = (1.0 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16)
    bet = (0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    xd, gd, btd, wd, bd = x.to(dev), gam.to(dev), bet.to(dev), w.to(dev), b.to(dev)
    assert ops._lib.lib().wg_gemm_skinny_ln_supported(M, N, K, K, K, N) == 1 and ops.gemm_route(xd, wd, bd, tile=5) == 5
    wt = ops.tile_weight(wd)
    NW = 16 if K >= 2048 and K % 512 == 0 else 4
    for ln, tiled, act, out_f32 in itertools.product((True, False), (False, True), (gr.ACT_NONE, gr.ACT_GELU), (False, True)):
        rd = gr.skinny_ln_reference(x, gam, bet, eps, w, b, act, NW) if ln else gr.reference(x, w, b, None, 0, act)
        out = ops.layernorm_linear(xd, gd if ln else None, btd if ln else None, eps, wd, bd, act=act, out_f32=out_f32, weight_tiled=wt if tiled else None)
        worst, share = gr.check(out, rd, K, act, False, out_f32, False)
        print("gemm bound: route 5 LN %d tiled %d M %d K %d act %d f32 %d: worst %.3f" % (ln, tiled, M, K, act, out_f32, worst))
        assert worst <= 1.0 and share == 0.0
