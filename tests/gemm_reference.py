"""Exact cases, float64 references and the per-element error bound for the bf16 GEMM forward kernels of csrc/gemm.hip (plain module, shared
by tests/test_gemm_check_host.py and tests/test_gpu_gemm_bounds.py).

Exact cases.  Integer operands held in bf16: A in [-3, 3], W in [-2, 2] with W[:, 0] += arange(N) % 5 (a transposed or permuted fragment
map cannot pass), integer bias in [-4, 4] and residual in [-8, 8].  Every product and partial sum is an integer below 2^24, so fp32
accumulation is exact in ANY order and the only arithmetic left is the rounding of the stored value, which the kernels state:
    unstaged epilogue (routes 3, 5, and 1 / 2 / 14 without the staged flag)    bf16(act(acc + b) + r), one rounding; none for fp32 outputs
    staged epilogue (11, 12, 16, and 1 / 2 / 14 with the flag)                 bf16(float(bf16(act(acc + b))) + r): wg_flush_slab adds the
                                                                               residual to the already rounded tile
`exact_expected` applies the model that ops.gemm_route's flag names; the comparison is torch.equal.  Activations: none and ReLU.
The LayerNorm-folded instance (17) has an exact case too: integer rows, integer Wg = bf16(W_int * gamma) with gamma = 1 + 2^-9 (the
product rounds back to W_int, so the unrounded W gamma has other row sums than Wg: what the column-sum mutant needs), integer colsum
and b', a small integer mean and a power-of-two rstd >= 1/8 per row: rstd * (x Wg^T - mean * s) + b' is then a multiple of 1/8 below
2^12, exact in fp32.

Random cases.  `reference` / `ln_reference` work in float64 on the operands as the kernel receives them (for the folded kernels Wg,
colsum, bias_f32 and the bf16 rows, not the unfolded layer) and return, with `pre` = act(acc + b) and `ref` = pre + r,
    S = sum_k |a_k w_k| + |b| (+ |r|)                                      plain kernels
    S = rstd * (sum_k |x_k wg_k| + |mean| |colsum|) + |b'|                 folded kernels.
The bound, one named term per rounding the code states, u = 2^-24:
    accumulation   c(K) u S L,   c(K) = 2 (K / 32 + 34).  The kernels add K / 32 MFMA results in sequence (one rounding of a partial sum each,
                   <= u S), every MFMA sums 32 exact products and the accumulator (any order: <= 32 u S_block, in total 32 u S), bias and
                   residual are one fp32 add each: K / 32 + 34.  The MFMA's internal order and intermediate width are not documented: factor
                   2.  The split-K kernels (skinny, row-wave) have fewer sequential steps than that.  The folded epilogue's four more fp32
                   operations (mean * rstd, * s, b' - ., the fma) are in LN_EPILOGUE_OPS.  L = 1.13 bounds the slope of GELU and
                   quick-GELU (1 for none / ReLU): the error reaches the output through the activation.
    activation     2.6e-5 for the fitted GELU (the project's figure: wg_act2e, tests/test_gpu_gemm_norm.py::
                   test_epilogue_gelu_through_an_identity_gemm); 2^-20 |pre| + 1e-7 for quick-GELU (v_exp_f32 and v_rcp_f32 are 1-ulp
                   approximations and the exp2 argument 2.46 x carries its own rounding: 16 fp32 ulps covers |x| <= 8; beyond, the
                   result is either x itself or below 1e-7); 0 for none / ReLU.
    bf16 rounding  half a bf16 step at the magnitude of the value being rounded, 2^(floor(log2 |v|) - 8), taken at |v| + the terms above:
                   once for the stored value, once more for `pre` when the staged epilogue adds a residual.  (Relative to the top of the
                   binade this is the 2^-9 per rounding of the attention bound; relative to |v| itself it reaches 2^-8 at v = 1 + 2^-8,
                   so `2^-9 |ref|` would refuse a correctly rounded result.)
    one-pass variance (kernel 17 fed by 18's partial sums, `stats_from_partials`): {sum x, sum x^2} per 256-column plane in fp32, any
                   order (<= 255 u sum|.|), np planes added in sequence, then / K, mean^2, the subtraction and + eps: cs = 256 + np + 4.
                   d_mean <= cs u mean|x|,  d_var <= cs u (mean(x^2) + 2 |mean| mean|x|),  d_rstd / rstd <= d_var / (2 (var + eps)) + 2 u
                   (v_rsq_f32: 1 ulp), and the output moves by  L (|pre-activation - b'| d_rstd / rstd + rstd |colsum| d_mean).
A kernel beyond the bound is a finding about the kernel; no factor is widened for it.

`emulate` / `ln_emulate`: what a faithful kernel computes, on the CPU in fp32 (64-deep slabs through torch's own matmul, added last slab
first: another order than the MFMA chain), the stated roundings, the statistics from fp32 partial sums.  `mutant=` gives deliberately wrong
kernels (GEMM_MUTANTS, LN_MUTANTS; the slab and bias mutants hit ONE tile, the last one).  tests/test_gemm_check_host.py holds the emulation
exact and inside the bound and every mutant not exact and, where random data shows it, outside the bound.

Measured, CPU (worst |out - ref| / bound over the shape families of tests/test_gemm_check_host.py): see MEASURED_CPU below.
Measured, MI355X: see MEASURED_GPU below; every case of tests/test_gpu_gemm_bounds.py prints its own (`gemm bound: route ... worst ...`, pytest -s).
"""
import math

import torch

U = 2.0 ** -24
GELU_FIT = 2.6e-5
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU = 0, 1, 2, 3
LN_EPILOGUE_OPS = 4
STAGED = 64                                     # ops.gemm_route's flag bit

GEMM_MUTANTS = ("slab_dropped", "slab_twice", "slabs_exchanged", "bias_next_tile", "res_wrap_off_by_one")
LN_MUTANTS = ("colsum_unrounded", "rstd_without_eps")

# worst |out - ref| / bound of the CPU emulation and of the mutants in random data (tests/test_gemm_check_host.py prints them with -s)
MEASURED_CPU = "emulation 0.974-0.998 (bf16 outputs: a rounding that lands on the half step), 0.004-0.023 (fp32 outputs), folded 0.965-0.995, " \
               "folded from partial sums 0.960-0.992; mutants: slab_dropped 39-1.3e5, slab_twice 41-1.3e5, slabs_exchanged 52-6.1e4, " \
               "bias_next_tile 3.7e3-1.3e5, res_wrap_off_by_one 9.8e3-1.1e5, colsum_unrounded 16-73, rstd_without_eps inf (the constant row: 0 * inf)"
MEASURED_GPU = "routes 1, 2, 3, 5, 11, 12, 14, 16, 17 (handed-in statistics) and 18 (output and partial planes): bit-exact on every exact case; random " \
               "data, bf16 outputs: routes 1 / 2 / 11 / 12 / 14 / 16 0.992-0.997, 17 0.992-0.996, 17 fed by 18 0.980-0.993, 5 0.725-0.994; fp32 " \
               "outputs: 1 and 14 0.011-0.018, 5 0.001-0.016 without and up to 0.515 with the LayerNorm (a normalised value one bf16 step from the " \
               "reference's)"


def acc_c(K):
    return 2.0 * (K // 32 + 34)


def _bf16(t):
    return t.to(torch.bfloat16)


def res_rows(M, res_mod):
    """Row of R that output row m reads."""
    m = torch.arange(M)
    return m % res_mod if res_mod > 0 else m


def exact_inputs(M, N, K, seed=1, rrows=None, bias=True):
    """a [M, K], w [N, K], b [N] or None, r [rrows, N] or None: small integers in bf16."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    w[:, 0] += torch.arange(N).float() % 5
    b = torch.randint(-4, 5, (N,), generator=g).float()
    r = torch.randint(-8, 9, (rrows or 1, N), generator=g).float()
    return _bf16(a), _bf16(w), (_bf16(b) if bias else None), (_bf16(r) if rrows else None)


def random_inputs(M, N, K, seed=2, rrows=None, bias=True):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    r = torch.randn(rrows or 1, N, generator=g)
    return _bf16(a), _bf16(w), (_bf16(b) if bias else None), (_bf16(r) if rrows else None)


def _act(y, act):
    if act == ACT_GELU:
        return torch.nn.functional.gelu(y)
    if act == ACT_QUICK_GELU:
        return y * torch.sigmoid(1.702 * y)
    if act == ACT_RELU:
        return torch.relu(y)
    return y


def _store(pre, radd, staged, out_f32):
    """The stated roundings on fp32 `pre` = act(acc + b) and the residual rows `radd` (fp32 or None)."""
    if out_f32:
        return pre if radd is None else pre + radd
    if radd is None:
        return _bf16(pre)
    return _bf16(_bf16(pre).float() + radd) if staged else _bf16(pre + radd)


def exact_acc(a, w):
    """a w^T of an exact case: the |a| |w|^T sums stay below 2^24, so fp32 is exact in any order (torch's included)."""
    assert (a.float().abs() @ w.float().abs().t()).max().item() < 2 ** 24 - 16
    return a.float() @ w.float().t()


def exact_expected(a, w, b, r, res_mod, act, staged, out_f32, acc=None):
    """acc: exact_acc(a, w), to share it between epilogues."""
    assert act in (ACT_NONE, ACT_RELU)
    acc = (exact_acc(a, w) if acc is None else acc).double()
    pre = _act(acc + (0 if b is None else b.double()), act).float()
    radd = None if r is None else r.float()[res_rows(a.shape[0], res_mod)]
    return _store(pre, radd, staged, out_f32)


def reference(a, w, b, r, res_mod, act):
    """-> dict(pre, ref, S, Sacc) float64 [M, N]."""
    ad, wd = a.double(), w.double()
    bd = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double()
    S = ad.abs() @ wd.abs().t() + bd.abs()
    pre = _act(ad @ wd.t() + bd, act)
    ref = pre
    if r is not None:
        rd = r.double()[res_rows(a.shape[0], res_mod)]
        ref, S = pre + rd, S + rd.abs()
    return {"pre": pre, "ref": ref, "S": S, "extra": torch.zeros_like(S)}


def half_step(v):
    """Half a bf16 step at the magnitude of v (float64)."""
    return v.abs().clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -8


def bound(rd, K, act, staged, out_f32, has_res, extra_ops=0):
    L = 1.13 if act in (ACT_GELU, ACT_QUICK_GELU) else 1.0
    e = (acc_c(K) + extra_ops) * U * rd["S"] * L + rd["extra"] * L
    if act == ACT_GELU:
        e = e + GELU_FIT
    elif act == ACT_QUICK_GELU:
        e = e + 2.0 ** -20 * rd["pre"].abs() + 1e-7
    if out_f32:
        return e + U * rd["ref"].abs()                        # (the fp32 store of the last add)
    if staged and has_res:
        e = e + half_step(rd["pre"].abs() + e)
    return e + half_step(rd["ref"].abs() + e)


def check(out, rd, K, act, staged, out_f32, has_res, extra_ops=0):
    """-> (worst |out - ref| / bound, share of elements beyond their bound); anything not finite counts as infinitely far off."""
    out = out.detach().double().cpu().reshape(rd["ref"].shape)
    ratio = (out - rd["ref"]).abs() / bound(rd, K, act, staged, out_f32, has_res, extra_ops)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    return ratio.max().item(), (ratio > 1).double().mean().item()


def _acc_fp32(a, w, bm, bn, mutant):
    """fp32 accumulators, 64-deep slabs added last slab first; the slab mutants act on the last (bm x bn) tile."""
    M, K = a.shape
    N = w.shape[0]
    nk = K // 64
    af, wf = a.float(), w.float()
    sl = lambda t, kt: t[:, 64 * kt:64 * kt + 64]
    acc = torch.zeros(M, N)
    for kt in reversed(range(nk)):
        acc += sl(af, kt) @ sl(wf, kt).t()
    if mutant in ("slab_dropped", "slab_twice", "slabs_exchanged"):
        m0, n0 = (M - 1) // bm * bm, (N - 1) // bn * bn
        kt = nk // 2 if mutant != "slabs_exchanged" else max(0, nk - 3)
        ta, tw = af[m0:], wf[n0:]
        if mutant == "slabs_exchanged":                      # A's slab kt meets W's slab kt + 2 and the other way round
            assert nk >= 3
            d = sl(ta, kt) @ sl(tw, kt + 2).t() + sl(ta, kt + 2) @ sl(tw, kt).t() - sl(ta, kt) @ sl(tw, kt).t() - sl(ta, kt + 2) @ sl(tw, kt + 2).t()
        else:
            d = sl(ta, kt) @ sl(tw, kt).t() * (-1.0 if mutant == "slab_dropped" else 1.0)
        acc[m0:, n0:] += d
    return acc


def emulate(a, w, b, r, res_mod, act, staged, out_f32, mutant=None, bm=256, bn=256):
    assert mutant is None or mutant in GEMM_MUTANTS
    M, N = a.shape[0], w.shape[0]
    acc = _acc_fp32(a, w, bm, bn, mutant)
    bf = torch.zeros(N) if b is None else b.float()
    if mutant == "bias_next_tile":
        n0 = (N - 1) // bn * bn
        assert b is not None and n0 > 0
        bf = bf.clone()
        bf[n0:] = bf[n0 - bn:n0 - bn + (N - n0)]            # the last column tile reads the bias of the tile before it
    pre = _act(acc + bf, act)
    radd = None
    if r is not None:
        rows = res_rows(M, res_mod)
        if mutant == "res_wrap_off_by_one":
            assert 0 < res_mod < M
            m = torch.arange(M)
            rows = torch.where(m >= res_mod, (rows + 1) % res_mod, rows)
        radd = r.float()[rows]
    return _store(pre, radd, staged, out_f32)


# ---- the LayerNorm-folded instances (17; 18 produces the partial sums) --------------------------------------------------------------

def fold(gamma, beta, w, b):
    """ops.fold_layernorm on the CPU: Wg = bf16(W gamma), colsum of the ROUNDED Wg (fp32), b' = b + W beta (fp32)."""
    wf = w.float()
    wg = _bf16(wf * gamma.float()[None, :])
    bp = wf @ beta.float()
    if b is not None:
        bp = bp + b.float()
    return wg, wg.float().sum(1), bp


def ln_exact_inputs(M, N, K, seed=3):
    """x [M, K] integer rows, wint [N, K], gamma [K], wg, colsum, bias_f32, stats [M rounded up to even, 2] = {small integer mean, power-of-two rstd},
    one pair per row, varied across rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (M, K), generator=g).float()
    wint = torch.randint(-2, 3, (N, K), generator=g).float()
    wint[:, 0] += torch.arange(N).float() % 5
    gamma = torch.full((K,), 1.0 + 2.0 ** -9)
    wg = _bf16(wint * gamma)
    colsum = wg.double().sum(1).float()
    bias_f32 = torch.randint(-4, 5, (N,), generator=g).float()
    m = torch.arange((M + 1) // 2 * 2)
    stats = torch.stack([((m * 7) % 5 - 2).float(), 2.0 ** -((m * 3) % 4).float()], 1).contiguous()
    return {"x": _bf16(x), "wint": wint, "gamma": gamma, "wg": wg, "colsum": colsum, "bias_f32": bias_f32, "stats": stats}


def ln_random_inputs(M, N, K, seed=4):
    """Rows with a mean of several sigma; row 1 at 30 sigma; rows 2, 3 near-constant and constant (variance ~ eps: rstd depends on eps)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + 3.0 * torch.randn(M, 1, generator=g)
    x[1] = 15.0 + 0.5 * torch.randn(K, generator=g)
    x[2] = 1.0 + 2.0 ** -7 * torch.randint(0, 2, (K,), generator=g).float()
    x[3] = 1.5
    gamma = _bf16(1.0 + 0.3 * torch.randn(K, generator=g))
    beta = _bf16(0.2 * torch.randn(K, generator=g))
    w = _bf16(torch.randn(N, K, generator=g) / K ** 0.5)
    b = _bf16(torch.randn(N, generator=g))
    wg, colsum, bias_f32 = fold(gamma, beta, w, b)
    return {"x": _bf16(x), "w": w, "gamma": gamma, "beta": beta, "wg": wg, "colsum": colsum, "bias_f32": bias_f32}


def row_stats64(x, eps):
    """{mean, rstd} of the stored rows in float64 -> [M, 2]."""
    xd = x.double()
    mean = xd.mean(1)
    return torch.stack([mean, (xd.var(1, unbiased=False) + eps).rsqrt()], 1)


def stats_fp32(x, eps):
    """The operand of wg_gemm_ln_bias_act_bf16: row_stats64 rounded to fp32, rows rounded up to even."""
    st = torch.zeros((x.shape[0] + 1) // 2 * 2, 2)
    st[:x.shape[0]] = row_stats64(x, eps).float()
    st[x.shape[0]:, 1] = 1.0
    return st


def ln_products(x, wg):
    """(x Wg^T, |x| |Wg|^T) in float64: the two matrix products of ln_reference, to share between activations."""
    return x.double() @ wg.double().t(), x.double().abs() @ wg.double().abs().t()


def ln_reference(x, wg, colsum, bias_f32, stats, act, from_partials=None, products=None):
    """stats [>= M, 2] as the kernel takes them (fp32 operand) or, for the partial-sum route, float64 statistics of the stored rows.
    from_partials = (np, eps): adds the one-pass variance term."""
    M, K = x.shape
    xd, sd, bd = x.double(), colsum.double(), bias_f32.double()
    xw, axw = products or ln_products(x, wg)
    mean, rstd = stats[:M, 0].double()[:, None], stats[:M, 1].double()[:, None]
    lin = rstd * (xw - mean * sd[None, :])
    S = rstd * (axw + mean.abs() * sd.abs()[None, :]) + bd.abs()
    pre = _act(lin + bd, act)
    extra = torch.zeros_like(S)
    if from_partials is not None:
        npl, eps = from_partials
        cs = 256 + npl + 4
        a1, q = xd.abs().mean(1, keepdim=True), (xd * xd).mean(1, keepdim=True)
        var = (q - mean * mean).clamp_min(0.0)
        d_mean = cs * U * a1
        d_rstd = cs * U * (q + 2 * mean.abs() * a1) / (2 * (var + eps)) + 2 * U
        extra = lin.abs() * d_rstd + rstd * sd.abs()[None, :] * d_mean
    return {"pre": pre, "ref": pre, "S": S, "extra": extra}


def ln_exact_expected(d, act):
    M = d["x"].shape[0]
    mean, rstd = d["stats"][:M, 0].double()[:, None], d["stats"][:M, 1].double()[:, None]
    v = rstd * (d["x"].double() @ d["wg"].double().t() - mean * d["colsum"].double()[None, :]) + d["bias_f32"].double()
    assert v.abs().max().item() < 2 ** 12 and bool((v * 8 == (v * 8).round()).all())
    return _bf16(_act(v, act).float())


def partials_fp32(x, mpad=None):
    """What kernel 18 leaves for rows x [M, np * 256]: [np][mpad][2] = {sum, sum of squares} per 256-column plane, fp32 sums."""
    M, K = x.shape
    mpad = mpad or (M + 255) // 256 * 256
    xt = x.float().view(M, K // 256, 256)
    part = torch.zeros(K // 256, mpad, 2)
    part[:, :M, 0] = xt.sum(-1).t()
    part[:, :M, 1] = (xt * xt).sum(-1).t()
    return part


def stats_from_partials(part, M, K, eps, mutant=None):
    S, Q = part[:, :M, 0].sum(0), part[:, :M, 1].sum(0)
    mean = S * (1.0 / K)
    var = (Q * (1.0 / K) - mean * mean).clamp_min(0.0)
    return torch.stack([mean, (var + (0.0 if mutant == "rstd_without_eps" else eps)).rsqrt()], 1)


def ln_emulate(x, wg, colsum, bias_f32, stats, act, mutant=None, unrounded=None):
    """stats: fp32 [>= M, 2].  mutant colsum_unrounded: the mean term takes the row sums of `unrounded` = W gamma before its rounding to bf16."""
    assert mutant is None or mutant in LN_MUTANTS
    M = x.shape[0]
    acc = _acc_fp32(x, wg, 256, 256, None)
    s = unrounded.float().sum(1) if mutant == "colsum_unrounded" else colsum
    r, mr = stats[:M, 1:2].float(), (stats[:M, 0:1] * stats[:M, 1:2]).float()
    return _bf16(_act(acc * r + (bias_f32[None, :] - mr * s[None, :]), act))


# ---- the skinny kernel with LayerNorm in front (route 5, LN = true) ----------------------------------------------------------------

def skinny_ln_reference(x, gamma, beta, eps, w, b, act, NW):
    """float64 LayerNorm -> bf16 rounding -> GEMM, with one more named term in `extra`: the kernel forms the normalised value in fp32, within
        d = cl u (|xn - beta| + rstd |gamma| mean|x|) + u |xn|,   cl = K / (4 NW) + NW + 12
    of the float64 one (row sums: K / (4 NW) sequential adds per lane, two swaps, NW partial sums; two exact passes, so the variance takes its
    summation error only relatively; sqrt, the division and the four operations of the affine map are in the 12), and an element whose
    float64 value lies within d of a bf16 rounding boundary may reach the MFMA one bf16 step away from the reference's:
        extra[m, n] = sum over those k of step(a[m, k]) |w[n, k]|.
    NW: the waves that split K (4, or 16 at K >= 2048 with K % 512 == 0)."""
    M, K = x.shape
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = (xd.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    gd, btd = gamma.double()[None, :], beta.double()[None, :]
    xn = (xd - mean) * rstd * gd + btd
    a = xn.to(torch.bfloat16)
    ad = a.double()
    cl = K // (4 * NW) + NW + 12
    d = cl * U * ((xn - btd).abs() + rstd * gd.abs() * xd.abs().mean(1, keepdim=True)) + U * xn.abs()
    hs = half_step(ad)
    pow2 = ad.abs() == ad.abs().clamp_min(2.0 ** -126).log2().floor().exp2()
    inward = (xn.abs() < ad.abs()) & pow2                    # below a power of two the step halves
    side = torch.where(inward, hs / 2, hs)
    may_flip = (side - (xn - ad).abs()) <= d
    rd = reference(a, w, b, None, 0, act)
    rd["extra"] = (may_flip.double() * 2 * side) @ w.double().abs().t()
    rd["flips"] = may_flip.double().mean().item()
    return rd
