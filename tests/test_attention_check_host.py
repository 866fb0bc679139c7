"""CPU checks (no GPU) of what tests/test_gpu_attention_bounds.py relies on: the error bound of tests/attn_reference.py accepts a faithful
bf16 emulation of the kernels' arithmetic and rejects every deliberately wrong reference, and the route queries of the library
(wg_mha_route / wg_sam_attn_route: host arithmetic) reach exactly the kernels listed here."""
import pytest
import torch

from tests import attn_reference as ar


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from walkgpt_amd import _lib
    h = _lib.lib()
    prev = h.wg_attn_pipe_mode(-1)
    yield h
    h.wg_attn_pipe_mode(prev)


_MHA_SHAPES = [(2, 100, 200, 2, 64, 3.0), (1, 97, 200, 2, 128, 3.0), (1, 100, 257, 2, 32, 3.0), (2, 7, 200, 2, 16, 3.0), (1, 100, 200, 2, 64, 1.0)]


@pytest.mark.parametrize("B,Lq,Lk,heads,hd,q_scale", _MHA_SHAPES)
def test_bound_accepts_the_emulation_and_rejects_every_mha_mutant(B, Lq, Lk, heads, hd, q_scale):
    """Around 100 x 200 keys.  Measured with these functions: the emulation at most 0.75 of the bound; the weakest mutant, the softmax scale
    off by 1 %, at least 2.8 times the bound at q x 3.  At q x 1 only the emulation is held to the bound: that the small faults hide there is
    the reason the GPU cases use q x 3 (tests/attn_reference.py)."""
    q, k, v = ar.mha_inputs(B, Lq, Lk, heads, hd, q_scale)
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(3)
    kb = torch.rand(B, Lk, generator=g) * 6.0 - 4.0                        # finite additive bias in [-4, 2]
    for bias in (None, kb):
        ref, A = ar.mha_reference(q, k, v, heads, scale, bias)
        assert (ref.abs() <= A + 1e-12).all()
        worst, share = ar.check(ar.mha_reference(q, k, v, heads, scale, bias, emulate=True)[0], ref, A)
        print("emulation %s bias: worst %.2f of the bound" % ("with" if bias is not None else "without", worst))
        assert worst <= 1.0 and share == 0.0, (worst, share)
        if q_scale < 3.0:
            continue
        for mutant in ar.MHA_MUTANTS:
            if mutant.startswith("bias") and bias is None:
                continue
            worst, share = ar.check(ar.mha_reference(q, k, v, heads, scale, bias, mutant=mutant)[0], ref, A)
            print("%-22s %s bias: worst %.1f x the bound, %.1f %% of the elements beyond it" % (mutant, "with" if bias is not None else "without", worst, 100 * share))
            assert worst > 1.0 and share > 0.0, (mutant, worst, share)


def test_bound_accepts_the_emulation_with_a_key_mask():
    """0 / finfo.min key masks as CLIP's padding mask makes them, the last 70 keys masked altogether."""
    B, Lq, Lk, heads, hd = 2, 65, 200, 2, 64
    q, k, v = ar.mha_inputs(B, Lq, Lk, heads, hd)
    keep = (torch.rand(B, Lk, generator=torch.Generator().manual_seed(8)) > 0.3).float()
    keep[:, 0] = 1
    keep[:, -70:] = 0
    kb = (1 - keep) * torch.finfo(torch.float32).min
    ref, A = ar.mha_reference(q, k, v, heads, hd ** -0.5, kb)
    assert torch.isfinite(ref).all()
    worst, share = ar.check(ar.mha_reference(q, k, v, heads, hd ** -0.5, kb, emulate=True)[0], ref, A)
    assert worst <= 1.0 and share == 0.0, (worst, share)
    unmasked, _ = ar.mha_reference(q, k, v, heads, hd ** -0.5, None)
    assert ar.check(unmasked, ref, A)[0] > 1.0


@pytest.mark.parametrize("B,grid,window,heads,hd", [(1, 15, 14, 2, 64), (2, 15, 14, 1, 32), (1, 15, 14, 1, 80), (1, 28, 14, 2, 32), (1, 15, 15, 1, 64)])
def test_bound_accepts_the_emulation_and_rejects_every_sam_mutant(B, grid, window, heads, hd):
    """A 15-grid in windows of 14 (padded to 28: one window holds a single real token).  Measured: the rel-pos mutants at least 23 times the
    bound.  The pad mutant applies only where the grid is not a multiple of the window."""
    qkv, bias, rel_h, rel_w = ar.sam_inputs(B, grid, window, heads, hd)
    ref, A = ar.sam_reference(qkv, bias, rel_h, rel_w, B, grid, window, heads)
    assert ref.shape == (B * grid * grid, heads * hd) and (ref.abs() <= A + 1e-12).all()
    worst, share = ar.check(ar.sam_reference(qkv, bias, rel_h, rel_w, B, grid, window, heads, emulate=True)[0], ref, A)
    print("emulation: worst %.2f of the bound" % worst)
    assert worst <= 1.0 and share == 0.0, (worst, share)
    for mutant in ar.SAM_MUTANTS:
        if mutant == "pad_kv_zero" and grid % window == 0:
            continue
        worst, share = ar.check(ar.sam_reference(qkv, bias, rel_h, rel_w, B, grid, window, heads, mutant=mutant)[0], ref, A)
        print("%-20s worst %.1f x the bound, %.1f %% of the elements beyond it" % (mutant, worst, 100 * share))
        assert worst > 1.0 and share > 0.0, (mutant, worst, share)


def test_sam_reference_is_the_existing_reference_in_float64():
    from tests.test_gpu_attention import _ref_sam_attention, _ref_mha
    qkv, bias, rel_h, rel_w = ar.sam_inputs(2, 15, 14, 2, 32)
    ref, _ = ar.sam_reference(qkv, bias, rel_h, rel_w, 2, 15, 14, 2)
    assert (ref - _ref_sam_attention(qkv, bias, rel_h, rel_w, 2, 15, 14, 2).double()).abs().max() < 1e-4
    q, k, v = ar.mha_inputs(2, 40, 70, 2, 32)
    kb = torch.rand(2, 70) - 0.5
    ref, _ = ar.mha_reference(q, k, v, 2, 0.2, kb)
    assert (ref - _ref_mha(q, k, v, 2, 0.2, kb).double()).abs().max() < 1e-4


def test_check_reports_how_far_off():
    ref = torch.tensor([[1.0, -2.0], [0.0, 0.5]], dtype=torch.float64)
    A = torch.tensor([[1.5, 2.0], [1.0, 0.5]], dtype=torch.float64)
    assert ar.check(ref.clone(), ref, A) == (0.0, 0.0)
    out = ref.clone()
    out[1, 0] = 3 * (2.0 ** -8 * 1.0 + 1e-6)            # three times this element's bound
    worst, share = ar.check(out, ref, A)
    assert abs(worst - 3.0) < 1e-9 and share == 0.25
    out[0, 1] = float("nan")
    worst, share = ar.check(out, ref, A)
    assert worst == float("inf") and share == 0.5
    assert ar.check(out.to(torch.bfloat16), ref, A)[0] == float("inf")


# ---- routes ---------------------------------------------------------------------------------------------------------------------------
T, W, U, P = 1, 2, 3, 4     # families of the route code: tiled, window, window-unit, pipe


def _code(family, hd, S, nw, kb=0):
    return family * 10000000 + hd * 10000 + S * 100 + nw * 10 + kb


# Every code wg_mha_route can return (with its negative answers) over Lq in 1..8192, per pipe mode.  A routing change has to edit this table.
# There is no eight-wave plain route at head_dim 32 or 64, tiled or pipe: four waves score 1.0 x their utilisation, eight 0.95 x a
# utilisation that is never higher (csrc/attn.hip, "compiled, not reachable from the entry point").
_PLAIN_TILED = {_code(T, hd, 0, nw, kb) for hd, nws in ((16, (1,)), (32, (1, 4)), (64, (1, 3, 4)), (128, (1, 4, 8))) for nw in nws for kb in (0, 1)}
_PLAIN_REACHABLE = {0: _PLAIN_TILED | {-2}, 1: _PLAIN_TILED | {-2}, 2: _PLAIN_TILED | {-2, _code(P, 64, 0, 4)}}
_SWEEP_LK = (40, 256, 257, 320, 1025)


def test_plain_routes_reachable_are_the_listed_ones(lib):
    for mode in (0, 1, 2):
        lib.wg_attn_pipe_mode(mode)
        seen = set()
        for hd in (16, 32, 64, 128):
            for kb in (0, 1):
                for Lk in _SWEEP_LK:
                    seen |= {lib.wg_mha_route(hd, Lq, Lk, kb) for Lq in range(1, 8193)}
        assert seen == _PLAIN_REACHABLE[mode], (mode, sorted(seen ^ _PLAIN_REACHABLE[mode]))
        for code in seen:
            if code > 0 and code // 10000 % 1000 in (32, 64):
                assert code // 10 % 10 != 8, code
    assert {lib.wg_mha_route(16, Lq, 100, 0) for Lq in range(33, 8193)} == {-2}          # head_dim 16: at most 32 queries
    assert lib.wg_mha_route(64, 0, 5, 0) == -1 and lib.wg_mha_route(48, 40, 40, 0) == -2


@pytest.mark.parametrize("hd,Lq,Lk,kb,modes,want", [
    (64, 33, 100, 0, (0, 1, 2), _code(T, 64, 0, 3)), (64, 65, 100, 0, (0, 1, 2), _code(T, 64, 0, 3)), (64, 96, 100, 0, (0, 1, 2), _code(T, 64, 0, 3)),
    (64, 97, 100, 0, (0, 1, 2), _code(T, 64, 0, 4)), (64, 32, 100, 1, (0, 1, 2), _code(T, 64, 0, 1, 1)),
    (128, 256, 100, 0, (0, 1, 2), _code(T, 128, 0, 8)), (128, 300, 100, 0, (0, 1, 2), _code(T, 128, 0, 4)), (32, 200, 100, 0, (0, 1, 2), _code(T, 32, 0, 4)),
    (64, 1025, 1025, 0, (0, 1), _code(T, 64, 0, 4)), (64, 1025, 1025, 0, (2,), _code(P, 64, 0, 4)), (64, 1025, 1025, 1, (2,), _code(T, 64, 0, 4, 1)),
    (64, 512, 256, 0, (2,), _code(P, 64, 0, 4)), (64, 512, 257, 0, (2,), _code(P, 64, 0, 4)), (64, 512, 320, 0, (2,), _code(T, 64, 0, 4)),
    (64, 512, 192, 0, (2,), _code(T, 64, 0, 4)), (64, 512, 258, 0, (2,), _code(T, 64, 0, 4)), (64, 20, 256, 0, (2,), _code(T, 64, 0, 1)),
])
def test_plain_route_of_named_shapes(lib, hd, Lq, Lk, kb, modes, want):
    for mode in modes:
        lib.wg_attn_pipe_mode(mode)
        assert lib.wg_mha_route(hd, Lq, Lk, kb) == want, mode


_SAM_ROUTES = [   # (B, grid, window, heads, head_dim) -> code under pipe mode 0, under modes 1 and 2
    ((1, 64, 64, 2, 64), _code(T, 64, 64, 8), _code(P, 64, 64, 8)),
    ((1, 64, 64, 2, 80), _code(T, 80, 64, 8), _code(T, 80, 64, 8)),
    ((1, 128, 64, 1, 64), _code(T, 64, 64, 8), _code(T, 64, 64, 8)),       # four 64 x 64 windows: not the pipelined kernel's case
    ((2, 64, 14, 3, 64), _code(U, 64, 14, 7), _code(U, 64, 14, 7)),
    ((1, 15, 14, 1, 64), _code(U, 64, 14, 7), _code(U, 64, 14, 7)),
    ((64, 64, 14, 64, 64), _code(W, 64, 14, 4), _code(W, 64, 14, 4)),      # an output of 2 GiB: past the unit kernel's 32-bit offsets
    ((1, 32, 32, 2, 64), _code(W, 64, 32, 8), _code(W, 64, 32, 8)),
    ((1, 29, 14, 1, 32), _code(W, 32, 14, 7), _code(W, 32, 14, 7)),
    ((1, 28, 28, 2, 32), _code(W, 32, 28, 5), _code(W, 32, 28, 5)),
    ((1, 64, 14, 2, 80), _code(W, 80, 14, 7), _code(W, 80, 14, 7)),
    ((1, 64, 16, 2, 64), -2, -2), ((1, 64, 14, 2, 128), -2, -2), ((1, 64, 64, 2, 32), -2, -2), ((1, 14, 28, 1, 32), -1, -1),
]


def test_sam_routes_are_the_listed_ones(lib):
    for mode in (0, 1, 2):
        lib.wg_attn_pipe_mode(mode)
        for args, off, on in _SAM_ROUTES:
            assert lib.wg_sam_attn_route(*args) == (off if mode == 0 else on), (mode, args)
    lib.wg_attn_pipe_mode(1)
    seen = {lib.wg_sam_attn_route(1, 64, w, 1, hd) for w in range(1, 65) for hd in (16, 32, 64, 80, 128)}
    assert seen == {-2, _code(U, 64, 14, 7), _code(W, 64, 32, 8), _code(P, 64, 64, 8), _code(W, 32, 14, 7), _code(W, 32, 28, 5), _code(W, 80, 14, 7),
                    _code(T, 80, 64, 8)}
    # the fp8 epilogue lives on the pipelined and the unit kernel
    assert [lib.wg_sam_attn_mx_supported(*a) for a in ((1, 64, 64, 2, 64), (1, 64, 14, 2, 64), (1, 64, 32, 2, 64), (1, 64, 64, 2, 80), (64, 64, 14, 64, 64))] \
        == [1, 1, 0, 0, 0]


def test_ops_route_wrappers_mirror_mha(lib):
    from walkgpt_amd import ops
    lib.wg_attn_pipe_mode(1)
    S = ops.ROUTE_SMALL
    assert ops.route_code(ops.ROUTE_TILED, 64, 0, 4, 1) == _code(T, 64, 0, 4, 1) and ops.route_code(ops.ROUTE_PIPE, 64, 64, 8) == _code(P, 64, 64, 8)
    assert ops.mha_route(32, 7, 7) == _code(S, 32, 0, 1) and ops.mha_route(16, 4096, 7) == _code(S, 16, 0, 1)       # few of either: one wave per query
    assert ops.mha_route(16, 7, 4096) == _code(T, 16, 0, 1) and ops.mha_route(64, 9, 257) == _code(T, 64, 0, 1)     # few queries, many keys: MFMA
    assert ops.mha_route(64, 9, 255) == _code(S, 64, 0, 1) and ops.mha_route(128, 40, 200, small=True) == _code(S, 128, 0, 1)
    assert ops.mha_route(128, 12, 4096, small=True) == _code(T, 128, 0, 1)       # (few queries, >= 256 keys: MFMA even where `small` is asked for)
    assert ops.mha_route(64, 5, 100, small=False) == _code(T, 64, 0, 1) and ops.mha_route(64, 65, 65, True) == _code(T, 64, 0, 3, 1)
    assert ops.mha_route(16, 100, 100) == _code(S, 16, 0, 1) and ops.mha_route(16, 100, 100, small=False) < 0 and ops.mha_route(64, 7, 7, True) < 0
    assert ops.sam_attention_route(1, 64, 64, 2, 64) == _code(P, 64, 64, 8)
