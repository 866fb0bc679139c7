"""Float64 references and the per-element error bound for the attention forward kernels (plain module, shared by
tests/test_attention_check_host.py and tests/test_gpu_attention_bounds.py).

The references
    mha_reference   softmax(scale q k^T + key_bias) v per head, any scale, optional additive key bias [B, Lk]
    sam_reference   SAM window / global attention on a packed qkv buffer, built like tests/test_gpu_attention.py's _ref_sam_attention:
                    positions that zero padding adds carry q = k = v = the qkv bias, oracle.sam.rel_pos_bias supplies the rel-pos term
work in float64 on the bf16-rounded inputs and return, with the output `ref`, the per-element quantity

    A = sum_j p_j |v_j|        (the same softmax weights applied to |V|; |ref| <= A)

The check: for every element   |out - ref| <= 2^-8 (|ref| + A) + 1e-6.

The factor is derived from the arithmetic the kernels state (attn.hip, attn_pipe.hip), not from a run:
    P is rounded to bf16 (v_cvt_pk_bf16_f32, nearest-even, relative error <= 2^-9) before P.V          <= 2^-9 A
    the row sum may be taken from the rounded P (attn_pipe.hip sums it on the matrix pipe)              <= 2^-9 |ref|
    the output is rounded to bf16                                                                       <= 2^-9 |ref|
together 2^-9 (A + 2 |ref|) <= 2^-9 A + 2^-8 |ref|; the 2^-9 A left over in the bound covers fp32 accumulation (scores over head_dim,
P.V over the keys, the running rescale) and the hardware exp2.  Scores, the rel-pos products and the key bias are fp32 in every kernel
(bf16 products are exact in fp32), so the bound has no further named term.  A kernel beyond the bound is a finding about the kernel; the
factor is not to be widened for it.

Inputs: bf16-rounded unit normal q, k, v with q scaled by 3 before rounding: rows are then peaked and outputs O(1), and a softmax scale
off by 1 % or one 64-key tile weighted 6 % too much lands at 3 to 7 times the bound.  With unit-scale q over thousands of keys (many small
weights: outputs average towards zero, A stays ~0.8) those two faults stay inside the bound, so q x 1 is only the second input set of
the long-loop cases.

`emulate=True` computes what a faithful kernel computes (fp32 scores, P rounded to bf16, the row sum from the unrounded P, a bf16 output);
`mutant=` gives deliberately wrong references.  tests/test_attention_check_host.py holds the emulation inside the bound and every mutant
outside it, on the CPU.

Measured (worst |out - ref| / bound): the CPU emulation 0.31-0.75 over the shapes of tests/test_attention_check_host.py; the weakest
mutant (scale x 0.99) 2.8-6.8, the tile mutant 6.5-7.5, the key-bias mutants 121-194, the rel-pos mutants 849-90199, the pad mutant 193-733.
The per-route figures of tests/test_gpu_attention_bounds.py on an MI355X are not recorded here yet: every case prints its own
(`attention bound: route ... worst ...`, pytest -s).
"""
import math

import torch

from oracle import sam as osam

FACTOR = 2.0 ** -8
FLOOR = 1e-6
LOG2E = 1.4426950408889634

MHA_MUTANTS = ("drop_last_key", "scale_x0.99", "tile_64_127_x1.0625", "bias_without_log2e", "bias_log2e_squared")
SAM_MUTANTS = ("rel_h_rel_w_swapped", "rel_h_row_zeroed", "pad_kv_zero")


def rand_bf16(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(torch.bfloat16)


def mha_inputs(B, Lq, Lk, heads, hd, q_scale=3.0, seed=40):
    """q [B, Lq, D], k, v [B, Lk, D]: bf16-rounded unit normals, q scaled by q_scale before the rounding."""
    D = heads * hd
    return rand_bf16((B, Lq, D), seed, q_scale), rand_bf16((B, Lk, D), seed + 1), rand_bf16((B, Lk, D), seed + 2)


def sam_inputs(B, grid, window, heads, hd, q_scale=3.0, seed=50):
    """qkv [B grid^2, 3D] (the q third scaled by q_scale before the rounding), the qkv bias [3D], rel_pos_h, rel_pos_w [2 window - 1, hd]."""
    D = heads * hd
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * grid * grid, 3 * D, generator=g)
    qkv[:, :D] *= q_scale
    return (qkv.to(torch.bfloat16), rand_bf16((3 * D,), seed + 1, 0.5), rand_bf16((2 * window - 1, hd), seed + 2, 0.2),
            rand_bf16((2 * window - 1, hd), seed + 3, 0.2))


def _softmax_pv(s, v, emulate, tile_mutant=False):
    """s [G, Lq, Lk] scores (natural-log domain), v [G, Lk, hd] -> (o, A), both [G, Lq, hd], in s's dtype."""
    p = (s - s.amax(-1, keepdim=True)).exp()
    if tile_mutant:
        p[..., 64:128] *= 1.0625
    l = p.sum(-1, keepdim=True)
    A = (p / l) @ v.abs()
    if emulate:
        p = p.to(torch.bfloat16).to(s.dtype)
    return (p @ v) / l, A


def mha_reference(q, k, v, heads, scale, key_bias=None, emulate=False, mutant=None):
    """-> (ref, A), float64 [B, Lq, D].  q [B, Lq, D], k / v [B, Lk, D] bf16; key_bias [B, Lk] fp32 additive or None."""
    assert mutant is None or mutant in MHA_MUTANTS
    B, Lq, D = q.shape
    hd = D // heads
    dt = torch.float32 if emulate else torch.float64
    sp = lambda t: t.to(dt).reshape(B, -1, heads, hd).transpose(1, 2).reshape(B * heads, -1, hd)
    Q, K, V = sp(q), sp(k), sp(v)
    kb = None if key_bias is None else key_bias.to(dt)
    if mutant == "drop_last_key":
        K, V = K[:, :-1], V[:, :-1]
        kb = None if kb is None else kb[:, :-1]
    if mutant == "scale_x0.99":
        scale = scale * 0.99
    if mutant == "bias_without_log2e":      # the exp2-domain score got `+ bias` where `+ bias * log2 e` belongs
        kb = kb / LOG2E
    if mutant == "bias_log2e_squared":
        kb = kb * LOG2E
    tile = mutant == "tile_64_127_x1.0625"
    assert not tile or K.shape[1] >= 128
    outs, As = [], []
    step = max(1, (1 << 25) // max(1, Lq * K.shape[1]))     # at most 2^25 scores at a time
    for g0 in range(0, B * heads, step):
        s = (Q[g0:g0 + step] @ K[g0:g0 + step].transpose(1, 2)) * scale
        if kb is not None:
            b_of = torch.arange(g0, min(g0 + step, B * heads)) // heads
            s = s + kb[b_of][:, None, :]
        o, A = _softmax_pv(s, V[g0:g0 + step], emulate, tile)
        outs.append(o)
        As.append(A)
    back = lambda t: torch.cat(t).reshape(B, heads, Lq, hd).transpose(1, 2).reshape(B, Lq, D)
    o, A = back(outs), back(As)
    if emulate:
        o = o.to(torch.bfloat16)
    return o.double(), A.double()


def sam_reference(qkv, bias, rel_h, rel_w, B, grid, window, heads, emulate=False, mutant=None):
    """-> (ref, A), float64 [B grid^2, D].  image_encoder.py:177-193 + 235-260 on an already-projected qkv buffer."""
    assert mutant is None or mutant in SAM_MUTANTS
    D = qkv.shape[-1] // 3
    hd = D // heads
    dt = torch.float32 if emulate else torch.float64
    rel_h, rel_w = rel_h.to(dt), rel_w.to(dt)
    if mutant == "rel_h_rel_w_swapped":
        rel_h, rel_w = rel_w, rel_h
    if mutant == "rel_h_row_zeroed":
        rel_h = rel_h.clone()
        rel_h[window] = 0                     # the row of query row = key row + 1
    pad = (-grid) % window
    assert mutant != "pad_kv_zero" or pad > 0
    Hp = grid + pad
    padrow = bias.to(dt) * (0.0 if mutant == "pad_kv_zero" else 1.0)
    full = padrow.reshape(1, 1, 1, 3 * D).repeat(B, Hp, Hp, 1)
    full[:, :grid, :grid] = qkv.to(dt).reshape(B, grid, grid, 3 * D)
    nw = Hp // window
    L = window * window
    w = full.reshape(B, nw, window, nw, window, 3 * D).permute(0, 1, 3, 2, 4, 5).reshape(-1, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = [t.reshape(-1, L, hd) for t in w]
    outs, As = [], []
    step = max(1, (1 << 25) // (L * L))
    for g0 in range(0, q.shape[0], step):
        qq = q[g0:g0 + step]
        s = (qq * hd ** -0.5) @ k[g0:g0 + step].transpose(1, 2) + osam.rel_pos_bias(qq, rel_h, rel_w, window)
        o, A = _softmax_pv(s, v[g0:g0 + step], emulate)
        outs.append(o)
        As.append(A)

    def back(t):
        t = torch.cat(t).reshape(B * nw * nw, heads, window, window, hd).permute(0, 2, 3, 1, 4).reshape(B, nw, nw, window, window, D)
        return t.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Hp, D)[:, :grid, :grid].reshape(B * grid * grid, D)

    o, A = back(outs), back(As)
    if emulate:
        o = o.to(torch.bfloat16)
    return o.double(), A.double()


def check(out, ref, A):
    """-> (worst |out - ref| / bound over the elements, share of the elements beyond their bound); bound = 2^-8 (|ref| + A) + 1e-6.
    A value above 1 in the first place is a failure and says by how much; anything that is not finite counts as infinitely far off."""
    out = out.detach().double().cpu().reshape(ref.shape)
    ratio = (out - ref).abs() / (FACTOR * (ref.abs() + A) + FLOOR)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    return ratio.max().item(), (ratio > 1).double().mean().item()
