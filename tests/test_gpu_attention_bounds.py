"""The attention forward kernels against float64 references under the per-element bound of tests/attn_reference.py
(|out - ref| <= 2^-8 (|ref| + A) + 1e-6, derived there), one case per route the entry points can take and per edge of it.

Every case (1) asserts the route code of the kernel it claims to exercise (ops.mha_route / ops.sam_attention_route: the decision the
launchers themselves use), (2) runs the kernel once, (3) applies the check and prints the worst ratio.  Inputs are q x 3 (peaked rows,
outputs O(1)) unless a case says q x 1.

Outside these cases, on purpose:
  * a key mask whose FIRST tile is wholly masked: key 0 stays valid in every mask here, as CLIP always keeps the class token; a row that
    starts with 64 masked keys is outside the kernels' contract;
  * wg_attn_window_kernel<64, 14, 4>: windows of 14 at head_dim 64 go to the unit kernel until the output passes 2 GiB (the route is
    asserted on the CPU, tests/test_attention_check_host.py); running it needs an output of that size;
  * the fp8 (MX) epilogue and the backward pass (tests/test_gpu_fp8.py, tests/test_gpu_backward.py).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_reference as ar
from tests.test_gpu_attention import pipe_plain  # noqa: F401  (fixture: plain attention may take the pipelined kernel, wg_attn_pipe_mode 2)
from walkgpt_amd import ops

T, W, U, P, SM = ops.ROUTE_TILED, ops.ROUTE_WINDOW, ops.ROUTE_WINDOW_UNIT, ops.ROUTE_PIPE, ops.ROUTE_SMALL
R = ops.route_code


@pytest.fixture
def pipe_off():
    """No case takes the pipelined kernel (wg_attn_pipe_mode 0): SAM's global attention runs on wg_attn_kernel<64, 64, 8>."""
    from walkgpt_amd import _lib
    prev = _lib.lib().wg_attn_pipe_mode(0)
    yield
    _lib.lib().wg_attn_pipe_mode(prev)


def _report(what, route, out, ref, A):
    worst, share = ar.check(out, ref, A)
    print("attention bound: route %d  %s  worst %.3f of the bound, %.4f of the elements beyond it" % (route, what, worst, share))
    assert worst <= 1.0, "%s on route %d: %.2f x the bound, %.2f %% of the elements beyond it" % (what, route, worst, 100 * share)


# ---- plain attention ------------------------------------------------------------------------------------------------------------------
def _key_bias(kind, B, Lk):
    if kind is None:
        return None
    g = torch.Generator().manual_seed(8)
    if kind == "finite":                                   # additive values in [-4, 2]: a bias at the wrong scale (a lost log2 e) shows
        return torch.rand(B, Lk, generator=g) * 6.0 - 4.0
    keep = (torch.rand(B, Lk, generator=g) > 0.3).float()  # "mask": CLIP's 0 / finfo.min key-padding mask
    if kind == "mask70":                                   # the last 70 keys masked: a wholly masked last tile and part of the one before
        keep = torch.ones(B, Lk)
        keep[:, -70:] = 0
    else:
        assert kind == "mask"
    keep[:, 0] = 1
    return (1 - keep) * torch.finfo(torch.float32).min


@functools.lru_cache(maxsize=None)
def _mha_case(B, Lq, Lk, heads, hd, scale, bias_kind, q_scale):
    q, k, v = ar.mha_inputs(B, Lq, Lk, heads, hd, q_scale)
    kb = _key_bias(bias_kind, B, Lk)
    ref, A = ar.mha_reference(q, k, v, heads, scale, kb)
    return q, k, v, kb, ref, A


def _run_mha(dev, route, B, Lq, Lk, heads, hd, scale_f=1.0, bias_kind=None, q_scale=3.0, small=False):
    scale = scale_f * hd ** -0.5
    q, k, v, kb, ref, A = _mha_case(B, Lq, Lk, heads, hd, scale, bias_kind, q_scale)
    assert ops.mha_route(hd, Lq, Lk, kb is not None, small) == route
    out = ops.mha(q.to(dev), k.to(dev), v.to(dev), heads, scale, None if kb is None else kb.to(dev), small=small)
    _report("mha B%d %dx%d heads %d hd%d scale x%.2f bias %s q x%g" % (B, Lq, Lk, heads, hd, scale_f, bias_kind, q_scale), route, out, ref, A)


@pytest.mark.parametrize("hd,Lq,Lk,route", [
    (64, 33, 100, R(T, 64, 0, 3)),     # one row in the last query block
    (64, 64, 100, R(T, 64, 0, 3)),     # whole blocks, one wave idle
    (64, 65, 100, R(T, 64, 0, 3)),
    (64, 96, 100, R(T, 64, 0, 3)),     # three whole blocks on three waves
    (64, 97, 100, R(T, 64, 0, 4)),     # four blocks: four waves
    (64, 130, 100, R(T, 64, 0, 3)),    # two workgroups, the second with one row in its last block
    (128, 256, 100, R(T, 128, 0, 8)),  # a multiple of eight query blocks at head_dim 128: eight waves
    (128, 300, 100, R(T, 128, 0, 4)),
    (32, 200, 100, R(T, 32, 0, 4)),
    (16, 7, 300, R(T, 16, 0, 1)),      # at most 32 queries on >= 256 keys: one MFMA wave per (batch, head)
    (32, 20, 300, R(T, 32, 0, 1)),
    (64, 32, 257, R(T, 64, 0, 1)),
    (128, 12, 256, R(T, 128, 0, 1)),
])
def test_plain_tiled_query_tails(dev, hd, Lq, Lk, route):
    _run_mha(dev, route, 1, Lq, Lk, 2, hd, small=None if Lq <= 32 else False)


@pytest.mark.parametrize("Lk", [40, 64, 65, 95, 96, 97, 127, 128, 257, 1025])
@pytest.mark.parametrize("hd,Lq,route", [(64, 70, R(T, 64, 0, 3)), (128, 40, R(T, 128, 0, 4)), (32, 40, R(T, 32, 0, 4))])
def test_plain_tiled_key_tails(dev, hd, Lq, route, Lk):
    """Fewer keys than one 64-key tile, exactly one tile, a tail of one key, tails on either side of the 32-key lane-half boundary."""
    _run_mha(dev, route, 1, Lq, Lk, 2, hd)


@pytest.mark.parametrize("hd,Lq,Lk,scale_f,route", [(16, 7, 300, 1.4, R(T, 16, 0, 1)), (32, 200, 100, 0.6, R(T, 32, 0, 4)), (64, 97, 100, 1.4, R(T, 64, 0, 4)),
                                                   (128, 256, 100, 0.6, R(T, 128, 0, 8))])
def test_plain_tiled_other_scale(dev, hd, Lq, Lk, scale_f, route):
    """A softmax scale that is not head_dim ** -0.5."""
    _run_mha(dev, route, 1, Lq, Lk, 2, hd, scale_f=scale_f, small=None if Lq <= 32 else False)


@pytest.mark.parametrize("bias_kind,Lk", [("finite", 200), ("mask", 200), ("mask70", 192), ("mask70", 198)])
@pytest.mark.parametrize("hd,Lq,route", [(16, 20, R(T, 16, 0, 1, 1)), (32, 200, R(T, 32, 0, 4, 1)), (32, 20, R(T, 32, 0, 1, 1)), (64, 65, R(T, 64, 0, 3, 1)),
                                         (64, 97, R(T, 64, 0, 4, 1)), (64, 20, R(T, 64, 0, 1, 1)), (128, 256, R(T, 128, 0, 8, 1)), (128, 300, R(T, 128, 0, 4, 1)),
                                         (128, 20, R(T, 128, 0, 1, 1))])
def test_plain_tiled_key_bias(dev, hd, Lq, route, bias_kind, Lk):
    """The additive key bias on every key-bias kernel: finite values in [-4, 2] (the kernels add it in the exp2 domain: the factor log2 e),
    CLIP's 0 / finfo.min mask, and a mask over the last 70 keys (192 keys: the last tile wholly masked and six keys of the tile before;
    198 keys: also a partial tile that is wholly masked).  Key 0 is always valid: a wholly masked first tile is outside the contract."""
    _run_mha(dev, route, 2, Lq, Lk, 2, hd, bias_kind=bias_kind)


@pytest.mark.parametrize("hd,Lq,L,route", [(64, 130, 130, R(T, 64, 0, 3)), (16, 20, 300, R(T, 16, 0, 1))])
def test_plain_packed_qkv_views(dev, hd, Lq, L, route):
    """q, k, v as column slices of one packed [B, L, 3D] buffer (CLIP's layout); the queries the first Lq rows of it."""
    B, heads = 2, 2
    D = heads * hd
    qkv = ar.rand_bf16((B, L, 3 * D), 60)
    qkv[..., :D] = (qkv[..., :D].float() * 3).to(torch.bfloat16)
    scale = hd ** -0.5
    ref, A = ar.mha_reference(qkv[:, :Lq, :D], qkv[..., D:2 * D], qkv[..., 2 * D:], heads, scale)
    d = qkv.to(dev)
    small = None if Lq <= 32 else False
    assert ops.mha_route(hd, Lq, L, False, small) == route
    out = ops.mha(d[:, :Lq, :D], d[..., D:2 * D], d[..., 2 * D:], heads, scale, small=small)
    _report("mha packed qkv B%d %dx%d hd%d" % (B, Lq, L, hd), route, out, ref, A)


@pytest.mark.parametrize("hd,Lq,Lk,route", [(64, 70, 100, R(T, 64, 0, 3)), (16, 7, 300, R(T, 16, 0, 1))])
def test_plain_shared_keys_zero_batch_stride(dev, hd, Lq, Lk, route):
    """K / V of one batch item shared by all (batch stride 0), as the mask decoder's first layer passes them."""
    B, heads = 3, 2
    q, k, v = ar.mha_inputs(B, Lq, Lk, heads, hd)
    k, v = k[:1], v[:1]
    scale = hd ** -0.5
    ref, A = ar.mha_reference(q, k.expand(B, -1, -1), v.expand(B, -1, -1), heads, scale)
    small = None if Lq <= 32 else False
    assert ops.mha_route(hd, Lq, Lk, False, small) == route
    kd, vd = k.to(dev).expand(B, -1, -1), v.to(dev).expand(B, -1, -1)
    assert kd.stride(0) == 0
    out = ops.mha(q.to(dev), kd, vd, heads, scale, small=small)
    _report("mha shared k/v B%d %dx%d hd%d" % (B, Lq, Lk, hd), route, out, ref, A)


@pytest.mark.parametrize("B,Lq,Lk,heads,route", [
    (1, 200, 256, 2, R(P, 64, 0, 4)),    # four tiles: the shortest loop the pipelined kernel takes
    (1, 200, 257, 2, R(P, 64, 0, 4)),    # ... and the lone 257th key
    (1, 200, 512, 2, R(P, 64, 0, 4)),
    (2, 97, 512, 3, R(P, 64, 0, 4)),     # batch and head decode
    (1, 200, 320, 2, R(T, 64, 0, 4)),    # an odd number of tiles: not the pipelined kernel's
    (1, 65, 256, 2, R(T, 64, 0, 3)),     # three waves: not the pipelined kernel's
])
def test_plain_pipelined(dev, B, Lq, Lk, heads, route, pipe_plain):
    """Plain attention under wg_attn_pipe_mode 2: wg_attn_pipe_kernel<0, 4> where the key count is an even number >= 4 of whole tiles (+ at
    most one lone key), the tiled kernel elsewhere."""
    _run_mha(dev, route, B, Lq, Lk, heads, 64)


@pytest.mark.parametrize("Lq,Lk,hd", [(7, 7, 32), (4, 1, 128), (4096, 7, 16), (5, 100, 64), (1, 33, 16)])
def test_one_wave_per_query(dev, Lq, Lk, hd):
    """wg_mha_small_bf16 (small=True): one wave per query; one lane per query where at most 32 keys meet many queries."""
    _run_mha(dev, R(SM, hd), 2, Lq, Lk, 2, hd, small=True)


@pytest.mark.parametrize("q_scale", [1.0, 3.0])
@pytest.mark.parametrize("hd,Lq,mode,route", [(64, 97, 1, R(T, 64, 0, 4)), (64, 97, 2, R(P, 64, 0, 4)), (16, 7, 1, R(T, 16, 0, 1)), (128, 12, 1, R(T, 128, 0, 1)),
                                              (128, 256, 1, R(T, 128, 0, 8))])
def test_long_loop_4096_keys(dev, hd, Lq, mode, route, q_scale):
    """64 tiles per row on the tiled, the pipelined and the one-wave MFMA routes; q x 1 (thousands of small weights) beside q x 3."""
    from walkgpt_amd import _lib
    prev = _lib.lib().wg_attn_pipe_mode(mode)
    try:
        _run_mha(dev, route, 1, Lq, 4096, 2, hd, q_scale=q_scale, small=None if Lq <= 32 else False)
    finally:
        _lib.lib().wg_attn_pipe_mode(prev)


# ---- SAM window / global attention ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sam_case(B, grid, window, heads, hd, q_scale=3.0):
    qkv, bias, rel_h, rel_w = ar.sam_inputs(B, grid, window, heads, hd, q_scale)
    ref, A = ar.sam_reference(qkv, bias, rel_h, rel_w, B, grid, window, heads)
    return qkv, bias, rel_h, rel_w, ref, A


def _run_sam(dev, route, B, grid, window, heads, hd, q_scale=3.0):
    qkv, bias, rel_h, rel_w, ref, A = _sam_case(B, grid, window, heads, hd, q_scale)
    assert ops.sam_attention_route(B, grid, window, heads, hd) == route
    out = ops.sam_attention(qkv.to(dev), bias.to(dev), rel_h.to(dev), rel_w.to(dev), B, grid, window, heads)
    _report("sam B%d grid %d window %d heads %d hd%d q x%g" % (B, grid, window, heads, hd, q_scale), route, out, ref, A)


@pytest.mark.parametrize("B,heads", [(1, 1), (2, 3)])
def test_sam_global_pipelined(dev, B, heads):
    """The 64 x 64 global grid at head_dim 64 under the default mode: wg_attn_pipe_kernel<64, 8>."""
    _run_sam(dev, R(P, 64, 64, 8), B, 64, 64, heads, 64)


@pytest.mark.parametrize("B,heads", [(1, 1), (2, 3)])
def test_sam_global_tiled_head_dim_64(dev, B, heads, pipe_off):
    """The same under wg_attn_pipe_mode 0: wg_attn_kernel<64, 64, 8, false> (the inputs and the reference are the pipelined case's)."""
    _run_sam(dev, R(T, 64, 64, 8), B, 64, 64, heads, 64)


def test_sam_global_head_dim_80(dev):
    _run_sam(dev, R(T, 80, 64, 8), 1, 64, 64, 1, 80)


def test_sam_global_many_small_weights(dev):
    """q x 1 on 4096 keys, the pipelined kernel."""
    _run_sam(dev, R(P, 64, 64, 8), 1, 64, 64, 1, 64, q_scale=1.0)


@pytest.mark.parametrize("grid", [15, 29, 64])
@pytest.mark.parametrize("hd,route", [(32, R(W, 32, 14, 7)), (64, R(U, 64, 14, 7)), (80, R(W, 80, 14, 7))])
def test_sam_windows_of_14(dev, hd, route, grid):
    """Grid 15 is padded to 28 (three of the four windows are almost all padding, one holds a single real token), 29 to 42, 64 to 70."""
    _run_sam(dev, route, 1, grid, 14, 2, hd)


@pytest.mark.parametrize("grid,window,hd,route", [(28, 28, 32, R(W, 32, 28, 5)), (32, 32, 64, R(W, 64, 32, 8))])
def test_sam_window_equal_to_the_grid(dev, grid, window, hd, route):
    _run_sam(dev, route, 1, grid, window, 2, hd)


@pytest.mark.parametrize("grid,window,hd,route", [(29, 14, 32, R(W, 32, 14, 7)), (29, 14, 64, R(U, 64, 14, 7)), (56, 28, 32, R(W, 32, 28, 5))])
def test_sam_windows_batch_and_heads(dev, grid, window, hd, route):
    """B = 2 with three heads, once per kernel family (the global kernels have theirs above): a wrong batch, window or head decode."""
    _run_sam(dev, route, 2, grid, window, 3, hd)
