"""Float64 references, fp32 emulations, mutants and tolerances for the mask-decoder kernels of walkgpt_amd/csrc/decoder.hip (plain module,
CPU only, shared by tests/test_decoder_host.py and tests/test_gpu_decoder_kernels.py), in the manner of tests/llm_reference.py.

Units (each a function of an `Arith`, the plain state_dict tensors `w` of a random-init MaskDecoder and plain tensors):
    tokens_reference        the stages of wg_dec_tokens_f32 in the kernel's order: INIT, SUM_MLP, SELF, Q_T2I, COMBINE
    attn_partial_reference  softmax(q k^T / 4) v over the hw image keys per (prompt, head, token); attn_partials / merge_partials: the ABI's
                            {m[6], l[6], o[6][16]} per (prompt, head, split of 1024 keys) and its merge
    mlp_partial_reference   slice s of the MLP: relu(x W1[s]^T + b1[s]) W2[:, s]^T
    heads_reference         hypernetwork i on token row 1 + i, the IoU head on row 0
    i2t_rows_reference      norm4(keys (+ res_bias) + out_proj(softmax(q k^T / 4) v)) over the six prompt tokens
    upscale_reference       ConvTranspose2d -> LayerNorm2d -> GELU -> ConvTranspose2d -> GELU -> hyper @ upscaled

`Arith()` is float64 on the bf16-rounded operands: the statement of what each stage computes (tests/test_decoder_host.py holds the chain of
the units equal to oracle/sam.py's decoder in float64).  `Arith(emulate=True)` computes in fp32 what the kernels state: the input of every
token-side Linear, of the i2t out_proj and of the upscaler's second GEMM staged as hi = bf16(v), lo = bf16(v - hi); fp32 accumulation; a
max-subtracted exp softmax; the A&S 7.1.26 erf; results that the ABI keeps in bf16 (k_i2t, v_i2t, the i2t rows, the ctp tail's row) are
returned BEFORE that rounding.  `order` = 1 .. 3 are other legitimate fp32 orderings of the same arithmetic (K reversed, 32-wide chunked
accumulation, exp through exp2); `mutant=` names a deliberately wrong computation (MUTANTS).

TOLERANCE.  A worst-case forward bound is useless through these chains (a linearised |W|-propagated bound for SELF is near 0.26 |ref|), so
the tolerance is formed from the reference side only, never from a GPU run:
    tol[row, :] = M * E_row  (+ 2^-8 |ref| where the output is bf16)
    E_row = max over the row (last dimension) of |emulation before its final rounding - float64|, floored at 2^-24 max |ref_row|
M is fixed per unit from CPU measurements (tests/test_decoder_host.py repeats them on the inputs of the GPU file and asserts the rule):
    R_order  = the largest |alt - float64| / E_row over the alternative orderings
    R_mutant = the smallest row-wise maximum of |mutant - float64| / E_row over every applicable mutant, every row of the outputs the
               mutant is judged on (MUTANTS: a mutant that moves one output is judged there) and every input set
    4 R_order <= M <= R_mutant / 4,   M = the smallest power of two >= 4 R_order, and at least 8
Measured on the CPU (inputs: the *_case functions below; x ~ N(0, 1) with an outlier channel of +8, weights of std 1 / sqrt(K)):
    unit     kernel                                   R_order   R_mutant (its mutant)               M    GPU worst |out - ref| / tol (MI355X)
    tokens   wg_dec_tokens_f32, every stage mask         1.51      281 (drop_lo)                     8    0.39 (fp32 outputs), 0.99 (k_i2t / v_i2t, bf16)
    attn     wg_dec_attn_partial_f32 + float64 merge     3.03     5680 (attn_drop_last_key, hw 4096) 16    0.18
    mlp      wg_dec_mlp_partial_f32                      1.73      313 (drop_lo)                     8    0.19
    heads    wg_dec_heads_f32                            1.78      319 (drop_lo)                     8    0.25
    i2t      wg_dec_i2t_rows_bf16                        1.60      292 (drop_lo)                     8    0.99 (bf16 output)
    upscale  wg_upscale_mask_bf16                        2.11      239 (drop_lo)                    16    0.16
Every other mutant stands at 1e4 or more.  Where the output is bf16 the 2^-8 |ref| rounding term dominates the tolerance and a correctly
rounded result reaches it (0.99); without its `lo` MFMAs in tok_mm the kernels stand at 47 .. 190 times the tolerance in every case that
goes through tok_mm, and the exact cases of tests/test_gpu_decoder_kernels.py fail as well (checked once on a scratch build).
"""
import math

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
UBF = 2.0 ** -8
U32 = 2.0 ** -24
TOK_SUM_MLP, TOK_SELF, TOK_Q_T2I, TOK_COMBINE, TOK_INIT = 1, 2, 4, 8, 16
SPLIT = 1024            # keys per attention split
PART = 6 * 18           # floats of one attention partial
TR = "md.transformer"

# unit -> M (see the table above)
M = {"tokens": 8, "attn": 16, "mlp": 8, "heads": 8, "i2t": 8, "upscale": 16}

# mutant -> (units it applies to, the outputs it is judged on or None for all of the unit's)
MUTANTS = {
    "drop_lo": (("tokens", "mlp", "heads", "i2t", "upscale"), None),
    "self_v_from_x_plus_pe": (("tokens",), ("queries",)),
    "skip_pe_flipped": (("tokens",), ("queries",)),
    "sum_mlp_k_without_pe": (("tokens",), ("k_i2t",)),
    "lin2_bias_missing": (("tokens",), ("k_i2t", "v_i2t")),
    "mlp_slice_dropped": (("mlp",), ("sum",)),
    "combine_no_rescale": (("tokens",), ("queries",)),
    "combine_norm_swapped": (("tokens",), ("queries",)),
    "heads_row_off_by_one": (("heads",), ("hyper",)),
    "i2t_keys_3_5_swapped": (("i2t",), None),
    "i2t_res_bias_missing": (("i2t",), None),
    "upscale_dy_dx_swapped": (("upscale",), None),
    "upscale_ln_over_256": (("upscale",), None),
    "attn_drop_last_key": (("attn",), None),
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------------------
def rand(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def rand_bf16(shape, seed, std=1.0):
    return rand(shape, seed, std).to(BF16)


def build_decoder(seed=0):
    """A random-init MaskDecoder (SAM's geometry) with seeded weights rounded to bf16: matrices of std 1 / sqrt(fan_in), LayerNorm gammas
    1 + 0.2 n, betas 0.1 n, every bias 0.1 n -- a dropped bias or a swapped gamma and beta cannot hide."""
    from torch import nn
    from walkgpt_amd.segment_anything.modeling import LayerNorm2d, MaskDecoder, TwoWayTransformer
    dec = MaskDecoder(num_multimask_outputs=3, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                      transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    g = torch.Generator().manual_seed(1000 + seed)
    n = lambda t, std: torch.randn(t.shape, generator=g) * std     # noqa: E731
    with torch.no_grad():
        for mod in dec.modules():
            if isinstance(mod, (nn.LayerNorm, LayerNorm2d)):
                mod.weight.copy_(1 + n(mod.weight, 0.2))
                mod.bias.copy_(n(mod.bias, 0.1))
            elif isinstance(mod, nn.Linear):
                mod.weight.copy_(n(mod.weight, mod.in_features ** -0.5))
                mod.bias.copy_(n(mod.bias, 0.1))
            elif isinstance(mod, nn.ConvTranspose2d):
                mod.weight.copy_(n(mod.weight, mod.in_channels ** -0.5))
                mod.bias.copy_(n(mod.bias, 0.1))
            elif isinstance(mod, nn.Embedding):
                mod.weight.copy_(n(mod.weight, 1.0))
    return dec.eval().to(BF16)


def weights(dec):
    """{"md." + state_dict name: float64 CPU tensor}: what the references read"""
    return {"md." + k: v.detach().double().cpu() for k, v in dec.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------
class Arith:
    def __init__(self, emulate=False, mutant=None, order=0):
        assert mutant is None or mutant in MUTANTS, mutant
        self.emulate, self.mutant, self.order = emulate or mutant is not None, mutant, order
        self.dt = torch.float32 if self.emulate else torch.float64

    def c(self, t):
        return None if t is None else t.to(self.dt)

    def stage(self, x):
        """the A operand of an MFMA: a bf16 hi + lo pair"""
        if not self.emulate:
            return x
        hi = x.to(BF16).float()
        return hi if self.mutant == "drop_lo" else hi + (x - hi).to(BF16).float()

    def mm(self, a, wt):
        """a [.., K] . wt [N, K]^T, accumulated in this arithmetic's order"""
        wt = self.c(wt)
        if self.order == 1:
            return a.flip(-1) @ wt.flip(-1).T
        if self.order == 2:
            acc = torch.zeros(a.shape[:-1] + (wt.shape[0],), dtype=self.dt)
            for k in range(0, a.shape[-1], 32):
                acc = acc + a[..., k:k + 32] @ wt[:, k:k + 32].T
            return acc
        return a @ wt.T

    def bmm(self, a, b):
        """a [.., R, K] @ b [.., K, N], accumulated in this arithmetic's order"""
        if self.order == 1:
            return a.flip(-1) @ b.flip(-2)
        if self.order == 2:
            acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=self.dt)
            for k in range(0, a.shape[-1], 32):
                acc = acc + a[..., k:k + 32] @ b[..., k:k + 32, :]
            return acc
        return a @ b

    def lin(self, x, w, name, staged=True):
        y = self.mm(self.stage(x) if staged else x, w[name + ".weight"])
        return y + self.c(w[name + ".bias"])

    def exp(self, x):
        if self.emulate and self.order == 3:
            return torch.exp2(x * 1.4426950408889634)
        return torch.exp(x)

    def softmax(self, s):
        if not self.emulate:
            return torch.softmax(s, -1)
        p = self.exp(s - s.amax(-1, keepdim=True))
        return p / p.sum(-1, keepdim=True)

    def ln(self, x, w, name, eps):
        g, b = self.c(w[name + ".weight"]), self.c(w[name + ".bias"])
        if not self.emulate:
            return F.layer_norm(x, (x.shape[-1],), g, b, eps)
        d = x - x.mean(-1, keepdim=True)
        return d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)) * g + b

    def gelu(self, x):
        if not self.emulate:
            return F.gelu(x)
        z = x * 0.70710678118654752440
        az = z.abs()
        t = 1.0 / (1.0 + 0.3275911 * az)
        p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
        erf = torch.copysign(1.0 - p * self.exp(-az * az), z)
        return 0.5 * x * (1.0 + erf)


def _heads(t, n):
    """[P, T, n * c] -> [P, n, T, c]"""
    return t.reshape(t.shape[0], t.shape[1], n, -1).transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# token -> image attention: partials and their merge
# ---------------------------------------------------------------------------------------------------------------------------------------
def _kv_heads(kv_img, P, prompt_image):
    """kv_img [1 | P | B, hw, 256] bf16, columns [K_h | V_h] per head -> float64 K, V [P, 8, hw, 16]"""
    kv = kv_img.double()
    if prompt_image is not None:
        kv = kv[prompt_image.long()]
    kv = kv.expand(P, -1, -1).reshape(P, kv.shape[1], 8, 2, 16)
    return kv[:, :, :, 0].transpose(1, 2), kv[:, :, :, 1].transpose(1, 2)


def attn_partials(q, kv_img, prompt_image=None, A=None):
    """The ABI's partials of exact arithmetic: [P, 8, ceil(hw / 1024), 108] = {m[6], l[6], o[6][16]} per (prompt, head, split), in A's dtype."""
    A = A or Arith()
    P = q.shape[0]
    K, V = _kv_heads(kv_img, P, prompt_image)
    hw = K.shape[2]
    if A.mutant == "attn_drop_last_key":
        hw -= 1
    qh = _heads(A.c(q) * 0.25, 8)                                         # [P, 8, 6, 16]
    out = []
    for s0 in range(0, K.shape[2], SPLIT):
        k, v = A.c(K[:, :, s0:min(s0 + SPLIT, hw)]), A.c(V[:, :, s0:min(s0 + SPLIT, hw)])
        if k.shape[2] == 0:
            out.append(torch.cat([torch.full((P, 8, 6), -1e30, dtype=A.dt), torch.zeros(P, 8, 6 + 96, dtype=A.dt)], -1))
            continue
        sc = qh @ k.transpose(2, 3)                                       # [P, 8, 6, n]
        m = sc.amax(-1)
        ol = A.bmm(A.exp(sc - m[..., None]), torch.cat([v, torch.ones_like(v[..., :1])], -1))       # o | l, summed over the keys in A's order
        out.append(torch.cat([m, ol[..., 16], ol[..., :16].reshape(P, 8, 96)], -1))
    return torch.stack(out, 2)


def merge_partials(partials, A=None):
    """o = sum_s o_s e^(m_s - M) / sum_s l_s e^(m_s - M) over the splits: [P, 8, S, 108] -> [P, 6, 128] (head h in columns 16 h ..)"""
    A = A or Arith()
    part = A.c(partials)
    P = part.shape[0]
    m, l, o = part[..., :6], part[..., 6:12], part[..., 12:].reshape(P, 8, -1, 6, 16)
    if A.mutant == "combine_no_rescale":
        wgt = torch.ones_like(m)
    else:
        wgt = A.exp(m - m.amax(2, keepdim=True))
    num = (o * wgt[..., None]).sum(2)
    den = (l * wgt).sum(2)
    return (num / den[..., None]).transpose(1, 2).reshape(P, 6, 128)


def attn_partial_reference(A, q, kv_img, prompt_image=None):
    """softmax(q k^T / 4) v over the hw keys per (prompt, head, token) (transformer.py:232-238) -> [P, 6, 128]"""
    if not A.emulate:
        K, V = _kv_heads(kv_img, q.shape[0], prompt_image)
        o = torch.softmax(_heads(q.double(), 8) @ K.transpose(2, 3) / 4.0, -1) @ V
        return o.transpose(1, 2).reshape(q.shape[0], 6, 128)
    return merge_partials(attn_partials(q, kv_img, prompt_image, A), Arith(emulate=True, order=A.order))


# ---------------------------------------------------------------------------------------------------------------------------------------
# token side
# ---------------------------------------------------------------------------------------------------------------------------------------
def ctp_tail_reference(A, x, gamma, beta, text_type, log_temp, eps):
    """normalize(LayerNorm(x) + text_type) * exp(log_temp) (utils_walkgpt.py:321-327), before the rounding to bf16"""
    x = A.c(x)
    d = x - x.mean(-1, keepdim=True)
    y = d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)) * A.c(gamma) + A.c(beta) + A.c(text_type)
    return y * (A.exp(A.c(log_temp)) / y.norm(dim=-1, keepdim=True).clamp_min(1e-12))


def tokens_reference(A, w, stages, skip_pe, queries=None, query_pe=None, self_blk=None, t2i=None, norm=None, sum_blk=None,
                     init_tokens=None, init_prompt=None, attn_part=None, attn_o=None, mlp_part=None, eps=1e-5):
    """The stages of wg_dec_tokens_f32 in the kernel's order.  self_blk / sum_blk: state_dict prefixes of TwoWayAttentionBlocks, t2i: of the
    token->image attention, norm: of the LayerNorm behind it (the operands of token_stage_table).  attn_part: the ABI's partials, or attn_o:
    the merged attention output [P, 6, 128].  -> dict of queries, query_pe, q_t2i, k_i2t, v_i2t (the last two BEFORE their bf16 rounding)."""
    mu = A.mutant
    out = {}
    if stages & TOK_INIT:                        # mask_decoder.py:125-132
        P = init_prompt.shape[0]
        x = torch.cat([A.c(init_tokens)[None].expand(P, -1, -1), A.c(init_prompt).reshape(P, 1, 256)], 1)
        pe = x.clone()
    else:
        x, pe = A.c(queries), A.c(query_pe)
    if mu == "skip_pe_flipped":
        skip_pe = not skip_pe
    if stages & TOK_SUM_MLP:                     # transformer.py:169-178
        x = x + A.c(mlp_part).sum(1)
        if mu != "lin2_bias_missing":
            x = x + A.c(w[sum_blk + ".mlp.lin2.bias"])
        x = A.ln(x, w, sum_blk + ".norm3", eps)
        i2t = sum_blk + ".cross_attn_image_to_token"
        out["k_i2t"] = A.lin(x if mu == "sum_mlp_k_without_pe" else x + pe, w, i2t + ".k_proj")
        out["v_i2t"] = A.lin(x, w, i2t + ".v_proj")
    if stages & TOK_SELF:                        # transformer.py:153-160
        sa = self_blk + ".self_attn"
        qk = x if skip_pe else x + pe
        q, k = A.lin(qk, w, sa + ".q_proj"), A.lin(qk, w, sa + ".k_proj")
        v = A.lin(x + pe if mu == "self_v_from_x_plus_pe" else x, w, sa + ".v_proj")
        p = A.softmax(_heads(q, 8) @ _heads(k, 8).transpose(2, 3) / math.sqrt(32))
        o = A.lin((p @ _heads(v, 8)).transpose(1, 2).reshape(x.shape), w, sa + ".out_proj")
        x = A.ln(o if skip_pe else x + o, w, self_blk + ".norm1", eps)
    if stages & TOK_Q_T2I:                       # transformer.py:162-165, :96-99
        out["q_t2i"] = A.lin(x + pe, w, t2i + ".q_proj")
    if stages & TOK_COMBINE:                     # out_proj, residual, norm2 / norm_final_attn
        o = A.c(attn_o) if attn_part is None else merge_partials(attn_part, A)
        x = x + A.lin(o, w, t2i + ".out_proj")
        x = A.ln(x, w, TR + ".layers.1.norm2" if mu == "combine_norm_swapped" else norm, eps)
    out["queries"], out["query_pe"] = x, pe
    return out


def mlp_partial_reference(A, w, blk, x, S):
    """slice s of mlp(x): relu(x W1[s]^T + b1[s]) W2[:, s]^T -> partials [P, S, 6, 256] and `sum` = their sum + lin2.bias (transformer.py:169)"""
    x = A.c(x)
    w1, b1, w2 = w[blk + ".mlp.lin1.weight"], A.c(w[blk + ".mlp.lin1.bias"]), w[blk + ".mlp.lin2.weight"]
    n = 2048 // S
    xs = A.stage(x)
    parts = []
    for s in range(S):
        hid = torch.relu(A.mm(xs, w1[s * n:(s + 1) * n]) + b1[s * n:(s + 1) * n])
        parts.append(A.mm(A.stage(hid), w2[:, s * n:(s + 1) * n]))
    part = torch.stack(parts, 1)
    total = part[:, :-1].sum(1) if A.mutant == "mlp_slice_dropped" else part.sum(1)
    return {"partials": part, "sum": total + A.c(w[blk + ".mlp.lin2.bias"])}


def _mlp3(A, w, prefix, x):
    x = torch.relu(A.lin(x, w, prefix + ".layers.0"))
    x = torch.relu(A.lin(x, w, prefix + ".layers.1"))
    return A.lin(x, w, prefix + ".layers.2")


def heads_reference(A, w, x):
    """mask_decoder.py:146-160: hypernetwork i on token row 1 + i -> hyper [P, 4, 32]; the IoU head on row 0 -> iou [P, 4]"""
    x = A.c(x)
    off = 0 if A.mutant == "heads_row_off_by_one" else 1
    hyper = torch.stack([_mlp3(A, w, "md.output_hypernetworks_mlps.%d" % i, x[:, off + i]) for i in range(4)], 1)
    return {"hyper": hyper, "iou": _mlp3(A, w, "md.iou_prediction_head", x[:, 0])}


# ---------------------------------------------------------------------------------------------------------------------------------------
# image side
# ---------------------------------------------------------------------------------------------------------------------------------------
def i2t_rows_reference(A, w, blk, q_img, k_i2t, v_i2t, keys, res_bias=None, prompt_image=None, eps=1e-5):
    """transformer.py:173-180: norm4(keys (+ res_bias) + out_proj(softmax(q k^T / 4) v)) over the six prompt tokens.  q_img [1 | P | B, hw, 128],
    keys [1 | P | B, hw, 256], k_i2t / v_i2t [P, 6, 128] -> [P, hw, 256] BEFORE the rounding to bf16."""
    P = k_i2t.shape[0]
    if prompt_image is not None:
        q_img, keys = q_img[prompt_image.long()], keys[prompt_image.long()]
    q, keys = A.c(q_img).expand(P, -1, -1), A.c(keys).expand(P, -1, -1)
    k, v = A.c(k_i2t), A.c(v_i2t)
    if A.mutant == "i2t_keys_3_5_swapped":
        k = k[:, [0, 1, 2, 5, 4, 3]]
    p = A.softmax(_heads(q * 0.25, 8) @ _heads(k, 8).transpose(2, 3))
    o = (p @ _heads(v, 8)).transpose(1, 2).reshape(P, -1, 128)
    name = blk + ".cross_attn_image_to_token.out_proj"
    bias = A.c(w[name + ".bias"])
    if res_bias is not None and A.mutant != "i2t_res_bias_missing":
        bias = bias + A.c(res_bias).reshape(-1)
    x = A.mm(A.stage(o), w[name + ".weight"]) + bias + keys
    return A.ln(x, w, blk + ".norm4", eps)


def upscale_reference(A, w, keys, hyper, h, wd, first_mask, num_masks):
    """mask_decoder.py:140-160 on a [P, 256, h, w] view of the token rows keys [P, h * w, 256]; hyper [P, 4, 32] -> [P, num_masks, 4h, 4w]"""
    P = keys.shape[0]
    w1, b1 = w["md.output_upscaling.0.weight"], w["md.output_upscaling.0.bias"]        # [Cin, Cout, 2, 2]
    w2, b2 = w["md.output_upscaling.3.weight"], w["md.output_upscaling.3.bias"]
    hy = A.c(hyper)[:, first_mask:first_mask + num_masks]
    if not A.emulate:
        from oracle.sam import _ln2d
        up = keys.double().transpose(1, 2).reshape(P, 256, h, wd)
        up = F.gelu(_ln2d(F.conv_transpose2d(up, w1, b1, stride=2), w, "md.output_upscaling.1"))
        up = F.gelu(F.conv_transpose2d(up, w2, b2, stride=2))
        return (hy @ up.flatten(2)).reshape(P, num_masks, 4 * h, 4 * wd)
    # the kernel's view: a k2 s2 transposed convolution is a per-token GEMM whose output columns are (dy, dx, c_out)
    x = A.c(keys).reshape(P * h * wd, 256)
    u = A.mm(x, w1.permute(2, 3, 1, 0).reshape(256, 256)).reshape(-1, 2, 2, 64) + A.c(b1)
    if A.mutant == "upscale_dy_dx_swapped":
        u = u.transpose(1, 2)
    g, b = A.c(w["md.output_upscaling.1.weight"]), A.c(w["md.output_upscaling.1.bias"])
    dims = (1, 2, 3) if A.mutant == "upscale_ln_over_256" else (3,)
    d = u - u.mean(dims, keepdim=True)
    u = A.gelu(d * (1.0 / torch.sqrt((d * d).mean(dims, keepdim=True) + 1e-6)) * g + b)
    z = A.mm(A.stage(u), w2.permute(2, 3, 1, 0).reshape(128, 64)).reshape(P, h * wd, 2, 2, 2, 2, 32) + A.c(b2)
    m = torch.einsum("pkc,ptabdec->pktabde", hy, A.gelu(z)).reshape(P, num_masks, h, wd, 2, 2, 2, 2)     # (ty, tx, dy, dx, dy2, dx2)
    return m.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(P, num_masks, 4 * h, 4 * wd)


# ---------------------------------------------------------------------------------------------------------------------------------------
# tolerance
# ---------------------------------------------------------------------------------------------------------------------------------------
def e_row(ref, emu):
    """E_row [.., 1]: the emulation's distance from float64 over each row, floored at 2^-24 max |ref_row|"""
    e = (emu.double() - ref).abs().amax(-1, keepdim=True)
    return torch.maximum(e, U32 * ref.abs().amax(-1, keepdim=True))


def tolerance(unit, ref, emu, bf16_out=False):
    tol = M[unit] * e_row(ref, emu).expand_as(ref)
    return tol + UBF * ref.abs() if bf16_out else tol


def check(out, ref, tol):
    """-> (worst |out - ref| / tol, share of the elements beyond it); anything not finite counts as infinitely far off"""
    out = out.detach().double().cpu().reshape(ref.shape)
    ratio = (out - ref).abs() / tol
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    return ratio.max().item(), (ratio > 1).double().mean().item()


def i2t_check(out, q_img, k_i2t, v_i2t, keys, out_w, out_b, ln_g, ln_b, eps, res_bias=None, prompt_image=None):
    """wg_dec_i2t_rows_bf16's output against the float64 reference on loose operands -> (worst ratio, share beyond), as `check`"""
    w = {"b.cross_attn_image_to_token.out_proj.weight": out_w, "b.cross_attn_image_to_token.out_proj.bias": out_b, "b.norm4.weight": ln_g,
         "b.norm4.bias": ln_b}
    w = {k: v.detach().double().cpu() for k, v in w.items()}
    cpu = lambda t: None if t is None else t.detach().cpu()     # noqa: E731
    ref, emu = (i2t_rows_reference(A, w, "b", cpu(q_img), cpu(k_i2t), cpu(v_i2t), cpu(keys), cpu(res_bias), cpu(prompt_image), eps)
                for A in (Arith(), Arith(emulate=True)))
    return check(out, ref, tolerance("i2t", ref, emu, True))


def row_ratio(alt, ref, emu):
    """row-wise maximum of |alt - float64| / E_row, flattened"""
    return ((alt.double() - ref).abs() / e_row(ref, emu)).amax(-1).flatten()


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the host and the GPU file
# ---------------------------------------------------------------------------------------------------------------------------------------
def token_rows(P, seed):
    """queries ~ N(0, 1) with an outlier channel of +8 (what a LayerNorm'd token stream carries), query_pe ~ N(0, 1): fp32, not bf16-representable"""
    x = rand((P, 6, 256), seed)
    x[..., 3] += 8
    return x, rand((P, 6, 256), seed + 1)


def attn_inputs(P, hw, kind, seed, n_img=None):
    """q [P, 6, 128] fp32, kv [n_img or P, hw, 256] bf16 in the interleaved [K_h | V_h] layout.  The six tokens of a (prompt, head) share a
    direction c, |c| = 4 (q = 2.6 c + 1.5 n per dimension: scores of std about 3 against N(0, 1) keys).
    kind "random": N(0, 1) keys; the LAST key is 2.5 c / |c| (score about 6.5 for every token), so losing it moves every output.
    kind "opposed": the keys of the first split are shifted by +20 c / |c|, all others by -20 c / |c|: scores about +52 and -52, per-split
    maxima about 100 apart."""
    n_img = n_img or P
    assert n_img in (1, P)
    c = rand((P, 8, 1, 16), seed)
    c = 4 * c / c.norm(dim=-1, keepdim=True)
    q = (2.6 * c + 1.5 * rand((P, 8, 6, 16), seed + 1)).transpose(1, 2).reshape(P, 6, 128).contiguous()
    k = rand((n_img, 8, hw, 16), seed + 2)
    v = rand((n_img, 8, hw, 16), seed + 3)
    cdir = (c / c.norm(dim=-1, keepdim=True))[:n_img]
    if kind == "random":
        k[:, :, -1:] = 2.5 * cdir
    else:
        sign = torch.where(torch.arange(hw) < SPLIT, 1.0, -1.0).reshape(1, 1, hw, 1)
        k = k + 20 * sign * cdir
    kv = torch.stack([k, v], 3).permute(0, 2, 1, 3, 4).reshape(n_img, hw, 256)
    return q, kv.to(BF16).contiguous()


def i2t_inputs(P, hw, seed, n_img=None):
    """q_img [n, hw, 128] (scores of std about 2), keys [n, hw, 256] with the outlier channel, k_i2t / v_i2t [P, 6, 128], res_bias [256]: bf16"""
    n = n_img or P
    keys = rand((n, hw, 256), seed + 1)
    keys[..., 3] += 8
    return dict(q_img=rand_bf16((n, hw, 128), seed, 2.0), keys=keys.to(BF16), k_i2t=rand_bf16((P, 6, 128), seed + 2),
                v_i2t=rand_bf16((P, 6, 128), seed + 3), res_bias=rand_bf16((256,), seed + 4, 0.5))


def upscale_inputs(P, h, wd, seed):
    keys = rand((P, h * wd, 256), seed)
    keys[..., 3] += 8
    return keys.to(BF16), rand((P, 4, 32), seed + 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tolerance cases: one list for the host file (emulation inside, mutants outside) and the GPU file (kernel inside)
# ---------------------------------------------------------------------------------------------------------------------------------------
L0, L1 = TR + ".layers.0", TR + ".layers.1"
T2I = ".cross_attn_token_to_image"
FINAL = TR + ".final_attn_token_to_image"


class Case:
    """unit, name, inputs (CPU tensors and plain values: what the GPU file feeds the kernel), fn(A, w) -> {output: tensor}, the outputs kept
    in bf16, the mutants that apply with the outputs each is judged on"""

    def __init__(self, unit, name, inputs, fn, bf16=(), mutants=None):
        self.unit, self.name, self.inputs, self.fn, self.bf16, self.mutants = unit, name, inputs, fn, tuple(bf16), dict(mutants or {})

    def __repr__(self):
        return "%s:%s" % (self.unit, self.name)

    def reference(self, w):
        """-> {output: (float64 reference, tolerance)}"""
        ref, emu = self.fn(Arith(), w), self.fn(Arith(emulate=True), w)
        return {k: (ref[k], tolerance(self.unit, ref[k], emu[k], k in self.bf16)) for k in ref}


def init_tokens(w):
    return torch.cat([w["md.iou_token.weight"], w["md.mask_tokens.weight"]], 0).float()


def _drop(out, *names):
    return {k: v for k, v in out.items() if k not in names}


def tokens_cases(w, P):
    x, pe = token_rows(P, 100 + P)
    mlp_part = rand((P, 16, 6, 256), 110 + P, 0.25)
    prompt = rand_bf16((P, 256), 120 + P)
    q, kv = attn_inputs(P, SPLIT + 16, "opposed", 130 + P)
    part = attn_partials(q, kv).float()
    lin = ("q_t2i", "k_i2t", "v_i2t", "queries")
    self_m = {"self_v_from_x_plus_pe": ("queries",), "skip_pe_flipped": ("queries",)}
    sum_m = {"sum_mlp_k_without_pe": ("k_i2t",), "lin2_bias_missing": ("k_i2t", "v_i2t")}
    mk = lambda name, stages, skip, ins, kw, lo, mut: Case(     # noqa: E731
        "tokens", "%s_P%d" % (name, P), dict(ins, stages=stages, skip_pe=skip, **kw),
        lambda A, w_: _drop(tokens_reference(A, w_, stages, skip, **ins, **kw), "query_pe"), ("k_i2t", "v_i2t"),
        dict(mut, drop_lo=lo))
    return [
        mk("init_self_q", TOK_INIT | TOK_SELF | TOK_Q_T2I, True, dict(init_tokens=init_tokens(w), init_prompt=prompt),
           dict(self_blk=L0, t2i=L0 + T2I, norm=L0 + ".norm2"), ("q_t2i", "queries"), self_m),
        mk("sum_self_q", TOK_SUM_MLP | TOK_SELF | TOK_Q_T2I, False, dict(queries=x, query_pe=pe, mlp_part=mlp_part),
           dict(self_blk=L1, t2i=L1 + T2I, norm=L1 + ".norm2", sum_blk=L0), lin, dict(self_m, **sum_m)),
        mk("sum_q", TOK_SUM_MLP | TOK_Q_T2I, False, dict(queries=x, query_pe=pe, mlp_part=mlp_part),
           dict(t2i=FINAL, norm=TR + ".norm_final_attn", sum_blk=L1), ("q_t2i", "k_i2t", "v_i2t"), sum_m),
        mk("self_q", TOK_SELF | TOK_Q_T2I, False, dict(queries=x, query_pe=pe),
           dict(self_blk=L1, t2i=L1 + T2I, norm=L1 + ".norm2"), ("q_t2i", "queries"), self_m),
        mk("combine", TOK_COMBINE, False, dict(queries=x, query_pe=pe, attn_part=part),
           dict(t2i=FINAL, norm=TR + ".norm_final_attn"), ("queries",), {"combine_no_rescale": ("queries",), "combine_norm_swapped": ("queries",)}),
        mk("sum", TOK_SUM_MLP, False, dict(queries=x, query_pe=pe, mlp_part=mlp_part), dict(sum_blk=L1), ("k_i2t", "v_i2t"), sum_m),
    ]


def attn_cases():
    out = []
    for hw, kind in ((48, "random"), (1024, "random"), (1040, "random"), (4096, "random"), (1040, "opposed")):
        q, kv = attn_inputs(2, hw, kind, 200 + hw)
        out.append(Case("attn", "%s_hw%d" % (kind, hw), dict(q=q, kv=kv), lambda A, w_, q=q, kv=kv: {"o": attn_partial_reference(A, q, kv)},
                        (), {"attn_drop_last_key": ("o",)} if kind == "random" else {}))
    return out


def chain_cases(w, P=2):
    """attention partials of the "opposed" set through the three consumers of COMBINE (the final attention's out_proj and norm_final_attn)"""
    q, kv = attn_inputs(P, SPLIT + 16, "opposed", 300)
    x, pe = token_rows(P, 310)
    kw = dict(t2i=FINAL, norm=TR + ".norm_final_attn")

    def combined(A, w_):
        A_ = Arith(emulate=A.emulate, order=A.order, mutant=A.mutant if A.mutant in ("drop_lo", "combine_no_rescale", "combine_norm_swapped") else None)
        return tokens_reference(A_, w_, TOK_COMBINE, False, queries=x, query_pe=pe, attn_o=attn_partial_reference(A_, q, kv), **kw)["queries"]

    ins = dict(q=q, kv=kv, queries=x, query_pe=pe, **kw)
    return [Case("tokens", "attn_combine", ins, lambda A, w_: {"queries": combined(A, w_)}, (), {"drop_lo": ("queries",)}),
            Case("mlp", "attn_combine_mlp", dict(ins, blk=L1), lambda A, w_: mlp_partial_reference(A, w_, L1, combined(A, w_), 16), (),
                 {"drop_lo": ("partials", "sum"), "mlp_slice_dropped": ("sum",)}),
            Case("heads", "attn_combine_heads", ins, lambda A, w_: heads_reference(A, w_, combined(A, w_)), (),
                 {"drop_lo": ("hyper", "iou"), "heads_row_off_by_one": ("hyper",)})]


def mlp_cases(P):
    x, _ = token_rows(P, 400 + P)
    return [Case("mlp", "P%d" % P, dict(x=x, blk=L0), lambda A, w_: mlp_partial_reference(A, w_, L0, x, 16), (),
                 {"drop_lo": ("partials", "sum"), "mlp_slice_dropped": ("sum",)})]


def heads_cases(P):
    x, _ = token_rows(P, 500 + P)
    return [Case("heads", "P%d" % P, dict(x=x), lambda A, w_: heads_reference(A, w_, x), (),
                 {"drop_lo": ("hyper", "iou"), "heads_row_off_by_one": ("hyper",)})]


def i2t_case(P, hw, form, bias, seed=600, blk=L0):
    """form: "prompt" (rows per prompt), "shared" (one image for all prompts), "map" (two images, prompt p reads image (p + 1) % 2)"""
    n = {"prompt": P, "shared": 1, "map": 2}[form]
    ins = i2t_inputs(P, hw, seed + P + hw, n)
    pimg = torch.tensor([(p + 1) % 2 for p in range(P)], dtype=torch.int32) if form == "map" else None
    rb = ins["res_bias"] if bias else None
    mut = {"drop_lo": ("keys",), "i2t_keys_3_5_swapped": ("keys",)}
    if bias:
        mut["i2t_res_bias_missing"] = ("keys",)
    fn = lambda A, w_: {"keys": i2t_rows_reference(A, w_, blk, ins["q_img"], ins["k_i2t"], ins["v_i2t"], ins["keys"], rb, pimg)}     # noqa: E731
    return Case("i2t", "P%d_hw%d_%s_%s" % (P, hw, form, "bias" if bias else "nobias"), dict(ins, res_bias=rb, prompt_image=pimg, blk=blk, P=P),
                fn, ("keys",), mut)


I2T_SHAPES = ((1, 16), (3, 64), (5, 1024))


def i2t_cases():
    return [i2t_case(P, hw, form, bias) for P, hw in I2T_SHAPES for form in ("prompt", "shared", "map") for bias in (False, True)
            if not (P == 1 and form == "shared")]


def i2t_loop_prompts(cus, hw=1040):
    """P such that P * hw rows exceed one trip of the persistent i2t kernel (128 rows per workgroup, one workgroup per CU) by one to two
    prompts' rows, less than a trip: 33 on 256 CUs"""
    return 128 * cus // hw + 2


UPSCALE_SHAPES = ((1, 4, 4), (2, 4, 12), (1, 8, 6), (3, 64, 64))
UPSCALE_MASKS = ((0, 1), (1, 3), (0, 4))


def upscale_case(P, h, wd):
    """all four masks; the GPU file slices the (first_mask, num_masks) ranges out of this one reference"""
    keys, hyper = upscale_inputs(P, h, wd, 700 + P + h + wd)
    return Case("upscale", "P%d_%dx%d" % (P, h, wd), dict(keys=keys, hyper=hyper, h=h, w=wd),
                lambda A, w_: {"masks": upscale_reference(A, w_, keys, hyper, h, wd, 0, 4)}, (),
                {"drop_lo": ("masks",), "upscale_dy_dx_swapped": ("masks",), "upscale_ln_over_256": ("masks",)})


def all_cases(w, big=True):
    cases = [c for P in (1, 5) for c in tokens_cases(w, P)] + attn_cases() + chain_cases(w)
    cases += [c for P in (1, 5) for c in mlp_cases(P) + heads_cases(P)] + i2t_cases()
    return cases + [upscale_case(*s) for s in UPSCALE_SHAPES if big or s[1] < 64]
