"""CPU checks of the GEMM test apparatus itself (tests/gemm_reference.py): the fp32 emulation of a faithful kernel reproduces the exact cases
bit for bit and stays inside the per-element bound on random data; every deliberately wrong kernel fails the exact comparison and, where
random data shows it, lies outside the bound.  The ratios printed here (-s) are the ones recorded in gemm_reference.MEASURED_CPU."""
import pytest
import torch

from tests import gemm_reference as gr

# (M, N, K, tile): ragged last row and column tiles, both parities of the slab count, one slab, many slabs
SHAPES = [(300, 272, 320, 128), (300, 272, 64, 128), (520, 520, 192, 256), (257, 264, 1024, 256), (300, 512, 128, 256)]
# (staged, out_f32, res_mod): res_mod None = no residual, 0 = one row per output row
EPILOGUES = [(True, False, None), (True, False, 0), (True, False, 100), (False, False, 0), (False, False, 100), (False, True, 0), (False, True, None)]
LN_SHAPES = [(300, 512, 256), (260, 256, 768), (257, 264, 1280)]


def _mutants_for(K, N, tile, res_mod, M):
    ms = ["slab_dropped", "slab_twice"]
    if K >= 192:
        ms.append("slabs_exchanged")
    if N > tile:
        ms.append("bias_next_tile")
    if res_mod:
        ms.append("res_wrap_off_by_one")
    return ms


@pytest.mark.parametrize("M,N,K,tile", SHAPES)
@pytest.mark.parametrize("staged,out_f32,res_mod", EPILOGUES)
def test_emulation_is_exact_and_every_mutant_is_not(M, N, K, tile, staged, out_f32, res_mod):
    rrows = None if res_mod is None else (res_mod or M)
    a, w, b, r = gr.exact_inputs(M, N, K, seed=M + K, rrows=rrows)
    for act in (gr.ACT_NONE, gr.ACT_RELU):
        want = gr.exact_expected(a, w, b, r, res_mod or 0, act, staged, out_f32)
        assert want.dtype == (torch.float32 if out_f32 else torch.bfloat16)
        assert torch.equal(gr.emulate(a, w, b, r, res_mod or 0, act, staged, out_f32, bm=tile, bn=tile), want)
        for mut in _mutants_for(K, N, tile, res_mod, M):
            assert not torch.equal(gr.emulate(a, w, b, r, res_mod or 0, act, staged, out_f32, mutant=mut, bm=tile, bn=tile), want), mut


def test_the_two_rounding_models_differ_on_the_exact_data():
    """The staged epilogue's second rounding is visible in the exact cases (so a test that applied the wrong model would fail)."""
    a, w, b, r = gr.exact_inputs(257, 264, 1024, seed=7, rrows=257)
    assert not torch.equal(gr.exact_expected(a, w, b, r, 0, gr.ACT_NONE, True, False), gr.exact_expected(a, w, b, r, 0, gr.ACT_NONE, False, False))


@pytest.mark.parametrize("M,N,K,tile", SHAPES)
@pytest.mark.parametrize("staged,out_f32,res_mod", EPILOGUES)
def test_emulation_inside_the_bound_and_visible_mutants_outside(M, N, K, tile, staged, out_f32, res_mod):
    rrows = None if res_mod is None else (res_mod or M)
    a, w, b, r = gr.random_inputs(M, N, K, seed=M + K + 1, rrows=rrows)
    for act in (gr.ACT_NONE, gr.ACT_GELU, gr.ACT_QUICK_GELU, gr.ACT_RELU):
        rd = gr.reference(a, w, b, r, res_mod or 0, act)
        args = (K, act, staged, out_f32, r is not None)
        worst, share = gr.check(gr.emulate(a, w, b, r, res_mod or 0, act, staged, out_f32, bm=tile, bn=tile), rd, *args)
        print("gemm bound (cpu): %s act %d staged %d f32 %d res %s emulation worst %.3f" % ((M, N, K), act, staged, out_f32, res_mod, worst))
        assert worst <= 1.0 and share == 0.0
        if act in (gr.ACT_NONE, gr.ACT_GELU):
            for mut in _mutants_for(K, N, tile, res_mod, M):       # every one of these is visible in random data
                mw, _ = gr.check(gr.emulate(a, w, b, r, res_mod or 0, act, staged, out_f32, mutant=mut, bm=tile, bn=tile), rd, *args)
                print("gemm bound (cpu):     mutant %s worst %.3g" % (mut, mw))
                assert mw > 1.0, mut


def test_bound_terms_are_what_the_docstring_states():
    assert gr.acc_c(64) == 2 * (2 + 34) and gr.acc_c(4096) == 2 * (128 + 34)
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.999, 2.0, -3.0, 0.75], dtype=torch.float64)
    assert torch.equal(gr.half_step(v), torch.tensor([2.0 ** -8] * 3 + [2.0 ** -7] * 2 + [2.0 ** -9], dtype=torch.float64))
    # a correctly rounded value reaches the half step and breaks `2^-9 |v|`
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20])
    err = (x.to(torch.bfloat16).double() - x.double()).abs()
    assert bool(err <= gr.half_step(x.double())) and bool(err > 2.0 ** -9 * x.double().abs())


@pytest.mark.parametrize("M,N,K", LN_SHAPES)
def test_folded_emulation_is_exact_and_every_mutant_is_not(M, N, K):
    d = gr.ln_exact_inputs(M, N, K, seed=M + K)
    assert len(set(map(tuple, d["stats"][:8].tolist()))) >= 6          # statistics vary from row to row
    for act in (gr.ACT_NONE, gr.ACT_RELU):
        want = gr.ln_exact_expected(d, act)
        assert torch.equal(gr.ln_emulate(d["x"], d["wg"], d["colsum"], d["bias_f32"], d["stats"], act), want)
        got = gr.ln_emulate(d["x"], d["wg"], d["colsum"], d["bias_f32"], d["stats"], act, mutant="colsum_unrounded", unrounded=d["wint"] * d["gamma"])
        assert not torch.equal(got, want)
        perm = d["stats"][:M].roll(1, 0)                                # a row-permuted statistics load
        assert not torch.equal(gr.ln_emulate(d["x"], d["wg"], d["colsum"], d["bias_f32"], perm, act), want)
    # statistics from partial sums, exactly: rows mean +- 1 (variance 1) with eps = 3 give rstd = 1/2; without eps, 1
    if K % 256 == 0:
        g = torch.Generator().manual_seed(K)
        sign = torch.cat([torch.ones(K // 2), -torch.ones(K // 2)])
        x = torch.stack([sign[torch.randperm(K, generator=g)] for _ in range(M)]) + d["stats"][:M, 0:1]
        d["x"] = x.to(torch.bfloat16)
        part = gr.partials_fp32(d["x"])
        st = gr.stats_from_partials(part, M, K, 3.0)
        assert torch.equal(st[:, 0], d["stats"][:M, 0]) and bool((st[:, 1] == 0.5).all())
        d["stats"] = st
        want = gr.ln_exact_expected(d, gr.ACT_NONE)
        assert torch.equal(gr.ln_emulate(d["x"], d["wg"], d["colsum"], d["bias_f32"], st, gr.ACT_NONE), want)
        bad = gr.stats_from_partials(part, M, K, 3.0, mutant="rstd_without_eps")
        assert not torch.equal(gr.ln_emulate(d["x"], d["wg"], d["colsum"], d["bias_f32"], bad, gr.ACT_NONE), want)


@pytest.mark.parametrize("M,N,K", LN_SHAPES)
def test_folded_emulation_inside_the_bound_and_mutants_outside(M, N, K):
    eps = 1e-6
    d = gr.ln_random_inputs(M, N, K, seed=M + K)
    ops4 = (d["x"], d["wg"], d["colsum"], d["bias_f32"])
    for act in (gr.ACT_NONE, gr.ACT_GELU, gr.ACT_QUICK_GELU):
        # statistics handed in (fp32 operand)
        st = gr.stats_fp32(d["x"], eps)
        rd = gr.ln_reference(*ops4, st, act)
        worst, share = gr.check(gr.ln_emulate(*ops4, st, act), rd, K, act, True, False, False, gr.LN_EPILOGUE_OPS)
        print("gemm bound (cpu): folded %s act %d emulation worst %.3f" % ((M, N, K), act, worst))
        assert worst <= 1.0 and share == 0.0
        mw, _ = gr.check(gr.ln_emulate(*ops4, st, act, mutant="colsum_unrounded", unrounded=d["w"].float() * d["gamma"].float()), rd, K, act, True, False,
                         False, gr.LN_EPILOGUE_OPS)
        print("gemm bound (cpu):     mutant colsum_unrounded worst %.3g" % mw)
        assert mw > 1.0
        # statistics from fp32 partial sums against float64 statistics of the rows
        if K % 256 == 0:
            part = gr.partials_fp32(d["x"])
            rd = gr.ln_reference(*ops4, gr.row_stats64(d["x"], eps), act, from_partials=(K // 256, eps))
            worst, share = gr.check(gr.ln_emulate(*ops4, gr.stats_from_partials(part, M, K, eps), act), rd, K, act, True, False, False, gr.LN_EPILOGUE_OPS)
            print("gemm bound (cpu): folded from partials %s act %d emulation worst %.3f" % ((M, N, K), act, worst))
            assert worst <= 1.0 and share == 0.0
            bad = gr.stats_from_partials(part, M, K, eps, mutant="rstd_without_eps")
            mw, _ = gr.check(gr.ln_emulate(*ops4, bad, act), rd, K, act, True, False, False, gr.LN_EPILOGUE_OPS)
            print("gemm bound (cpu):     mutant rstd_without_eps worst %.3g" % mw)
            assert mw > 1.0
