"""Float64 references and per-element error bounds for the LLaMA kernels of walkgpt_amd/csrc/llama.hip (plain module, shared by
tests/test_llm_host.py and tests/test_gpu_llm.py), in the manner of tests/attn_reference.py.

Attention (prefill and decode): `attn_reference` returns (ref, A) in attn_reference's form; its `check` and FACTOR are reused unchanged.
The prefill kernel states the arithmetic that bound was derived for (fp32 scores, P rounded to bf16 before P.V, the row sum from the
unrounded P, a bf16 output); the decode kernel keeps P in fp32, i.e. has one term fewer.

Every other kernel: `bound_check(out, ref, bound)` with a bound derived below from the arithmetic the kernel states, never from a run.
u = 2^-24 is the fp32 unit roundoff.  The bf16 one is 2^-8: bf16 keeps 8 significant bits (7 stored), so round-to-nearest moves a value by up
to half a unit in the last place, 2^-8 / (1 + 2^-8) of the value just above a power of two.  (A 2^-9 |ref| rounding term, the figure
tests/attn_reference.py quotes per rounding, holds only on average: a correctly rounded result reaches 1.99 times it, and the first run of
the RMSNorm kernel, which rounds once, stood at 1.88.  attn_reference's own bound is unaffected, its factor is 2^-8 on |ref| + A >= 2 |ref|.)

GEMV (wg_llama_gemv_bf16).  The kernel states: the normalised input xh = x * rstd * gamma stays fp32 (NOT rounded to bf16, so there is no
2^-8 sum |xh_k w_k| term); a lane adds its K / 64 products one after the other and the wave adds the 64 lane sums by a 6-level butterfly; the
only rounding to bf16 is that of the output.  With S = sum_k |xh_k w_k|:
    output rounding                2^-8 |ref|      (2^-24 |ref| for the fp32 output)
    fp32 accumulation              (K / 64 + 6) u S           every product passes through at most K / 64 + 6 additions
    xh itself                      (K / 256 + 16) u S         two multiplies (2 u) and rstd: a sum of K squares of which a thread adds K / 256,
                                                              then 6 + 2 levels, a division, a square root and a reciprocal (<= 6 u under fast-math)
    together                       E = (K / 64 + K / 256 + 22) u S, taken as (K / 64 + K / 256 + 32) u S
    residual   out = bf16(res + acc): 2^-8 |ref| + E + u |ref|
    pair       out = bf16(silu(g) * t): |silu'| <= 1.1, so 1.1 E_g |t| + |silu(g)| E_t, plus 8 u |ref| for the exponential, the division and
               the product, plus 2^-8 |ref|
RMSNorm (wg_rmsnorm_rows_bf16): fp32 throughout, one rounding: 2^-8 |ref| + (D / 256 + 16) u |ref|.
RoPE (wg_llama_rope_cache_bf16): fp32 tables (relative error <= 2 u against float64 cos / sin of the fp32 angle -- the references below take the
    SAME fp32 angle), out = bf16(a c -/+ b s): 2^-8 |ref| + 4 u (|a c| + |b s|).  v is a copy: exact.

`emulate_*` compute what a faithful kernel computes (fp32, the stated roundings); `mutant=` gives deliberately wrong results.
tests/test_llm_host.py holds every emulation inside its bound and every mutant outside it, on the CPU."""
import math

import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -8
BF16 = torch.bfloat16

TINY = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, rms_norm_eps=1e-5,
            max_position_embeddings=2048)


def tiny_config(vocab=96, **over):
    from transformers import LlamaConfig
    kw = dict(TINY, vocab_size=vocab)
    kw.update(over)
    return LlamaConfig(**kw)


def tiny_llm(vocab=96, seed=0, dtype=BF16, **over):
    """A random-init LlamaForCausalLM of the tiny config with bf16-rounded weights (kept in `dtype`)."""
    from transformers import LlamaForCausalLM
    torch.manual_seed(seed)
    llm = LlamaForCausalLM(tiny_config(vocab, **over)).eval()
    llm.to(BF16)
    return llm.to(dtype)


def rand_bf16(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF16)


def bound_check(out, ref, bound):
    """-> (worst |out - ref| / bound, share of the elements beyond it); anything not finite counts as infinitely far off."""
    out = out.detach().double().cpu().reshape(ref.shape)
    ratio = (out - ref).abs() / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    return ratio.max().item(), (ratio > 1).double().mean().item()


# ---- attention ------------------------------------------------------------------------------------------------------------------------
ATTN_MUTANTS = ("causal_off_by_one", "mask_other_row")


def attn_mask_rows(rows, Lk):
    """The key mask of the tests: everything attended, except row 1's keys 5 .. 18; key 0 is never masked."""
    m = torch.ones(rows, Lk, dtype=torch.bool)
    if rows > 1:
        m[1, 5:19] = False
    return m


def attn_reference(q, k, v, heads, mask, past=0, emulate=False, mutant=None):
    """softmax(q k^T / sqrt(128) + causal + key mask) v.  q [rows, L, H]; k, v [rows, Lk >= past + L, H] bf16; mask [rows, Lk] bool (True =
    attend); query j sits at position past + j and sees the keys <= its position.  -> (ref, A) float64 [rows, L, H]."""
    assert mutant is None or mutant in ATTN_MUTANTS
    rows, L, H = q.shape
    Lk, hd = k.shape[1], H // heads
    dt = torch.float32 if emulate else torch.float64
    sp = lambda t: t.to(dt).reshape(rows, -1, heads, hd).transpose(1, 2)               # [rows, heads, *, hd]
    Q, K, V = sp(q), sp(k), sp(v)
    qpos = past + torch.arange(L)
    if mutant == "causal_off_by_one":
        qpos = qpos + 1
    see = torch.arange(Lk)[None, :] <= qpos[:, None]                                    # [L, Lk]
    km = mask.roll(1, 0) if mutant == "mask_other_row" else mask
    ok = see[None, None] & km[:, None, None, :]
    s = (Q @ K.transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~ok, -math.inf)
    p = (s - s.amax(-1, keepdim=True)).exp()
    l = p.sum(-1, keepdim=True)
    A = (p / l) @ V.abs()
    if emulate:
        p = p.to(BF16).to(dt)
    o = (p @ V) / l
    back = lambda t: t.transpose(1, 2).reshape(rows, L, H)
    o, A = back(o), back(A)
    if emulate:
        o = o.to(BF16)
    return o.double(), A.double()


# ---- GEMV -----------------------------------------------------------------------------------------------------------------------------
GEMV_MUTANTS = ("drop_k_block", "eps_outside_sqrt", "gate_up_swapped")


def _normed(x, gamma, eps, dt, mutant=None):
    x = x.to(dt)
    if gamma is None:
        return x
    ms = (x * x).mean(-1, keepdim=True)
    rstd = 1.0 / (ms.sqrt() + eps) if mutant == "eps_outside_sqrt" else 1.0 / (ms + eps).sqrt()
    return x * rstd * gamma.to(dt)


def gemv_reference(x, weights, gamma=None, eps=0.0, residual=None, pair=False, out_f32=False, mutant=None, emulate=False):
    """x [M, K] bf16; weights: one to three [N_i, K] bf16 whose outputs sit side by side (pair: silu(W_0 xh) * (W_1 xh)).
    -> (ref, bound) float64 [M, N]; emulate: the kernel's arithmetic in fp32 with its output rounding (bound still from float64)."""
    assert mutant is None or mutant in GEMV_MUTANTS
    M, K = x.shape
    xh = _normed(x, gamma, eps, torch.float64, mutant)
    ws = [w.double() for w in weights]
    if mutant == "drop_k_block":
        ws = [w.clone() for w in ws]
        for w in ws:
            w[:, K - 128:] = 0
    if mutant == "gate_up_swapped":
        assert pair
        ws = ws[::-1]
    E = lambda w: (K / 64 + K / 256 + 32) * U32 * (xh.abs() @ w.abs().T)
    uo = U32 if out_f32 else UBF
    if pair:
        g, t = xh @ ws[0].T, xh @ ws[1].T
        silu = g / (1 + (-g).exp())
        ref = silu * t
        bound = 1.1 * E(ws[0]) * t.abs() + silu.abs() * E(ws[1]) + 8 * U32 * ref.abs()
    else:
        W = torch.cat(ws, 0)
        ref = xh @ W.T
        bound = E(W)
    if residual is not None:
        ref = ref + residual.double()
        bound = bound + U32 * ref.abs()
    bound = bound + uo * ref.abs()
    if emulate:
        assert mutant is None
        xf = _normed(x, gamma, eps, torch.float32)
        fs = [w.float() for w in weights]
        if pair:
            g, t = xf @ fs[0].T, xf @ fs[1].T
            o = g / (1 + (-g).exp()) * t
        else:
            o = xf @ torch.cat(fs, 0).T
        if residual is not None:
            o = o + residual.float()
        ref = (o if out_f32 else o.to(BF16)).double()
    return ref, bound


def rmsnorm_reference(x, w, eps, emulate=False):
    D = x.shape[-1]
    ref = _normed(x, w, eps, torch.float64)
    bound = (UBF + (D / 256 + 16) * U32) * ref.abs() + 1e-30
    if emulate:
        ref = _normed(x, w, eps, torch.float32).to(BF16).double()
    return ref, bound


# ---- RoPE -----------------------------------------------------------------------------------------------------------------------------
def rope_reference(x, positions, theta=10000.0, pairing="half", emulate=False):
    """x [..., T, heads * 128] bf16 rotated at integer `positions` [T].  pairing "half": (i, i + 64), transformers' rotate_half;
    "interleaved": (2i, 2i + 1), the mutant.  The angle is the fp32 product position * inv_freq that LlamaRotaryEmbedding forms.
    -> (ref, bound) float64."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    ang = (positions.float()[:, None] * inv_freq[None, :]).double()                    # [T, 64]
    dt = torch.float32 if emulate else torch.float64
    c, s = ang.cos().to(dt), ang.sin().to(dt)
    shp = x.shape
    xv = x.to(dt).reshape(shp[:-1] + (-1, 128))                                          # [..., T, heads, 128]
    c, s = c[:, None, :], s[:, None, :]
    if pairing == "half":
        a, b = xv[..., :64], xv[..., 64:]
        ref = torch.cat([a * c - b * s, b * c + a * s], -1)
        mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    else:
        a, b = xv[..., 0::2], xv[..., 1::2]
        ref = torch.stack([a * c - b * s, b * c + a * s], -1).flatten(-2)
        mag = torch.stack([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1).flatten(-2)
    ref, mag = ref.reshape(shp).double(), mag.reshape(shp).double()
    bound = UBF * ref.abs() + 4 * U32 * mag + 1e-30
    if emulate:
        ref = ref.to(BF16).double()
    return ref, bound


# ---- the token pick and the host's stop rule -----------------------------------------------------------------------------------------------
def pick_reference(logits, finished, eos, pad):
    """One step of the rule at walkgptForCausalLM._generate: argmax (lowest index on a tie), a finished row emits pad, finished |= token == eos.
    logits [rows, V]; finished: list of bool, updated in place.  -> list of token ids."""
    out = []
    for r in range(logits.shape[0]):
        row = logits[r]
        t = int((row == row.max()).nonzero()[0])
        if eos is not None:
            if finished[r]:
                t = pad
            finished[r] = finished[r] or t == eos
        out.append(t)
    return out
