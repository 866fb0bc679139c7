"""The e4m3 weight-only mode of the HIP LLaMA path (plain module, shared by tests/test_fp8w_host.py and tests/test_gpu_llm_fp8w.py): the torch
reference of the quantisation format, the test weights, and the GEMV mutants of this mode, in the manner of tests/llm_reference.py.

Format (include/walkgpt_hip.h).  For W [N, K] bf16 and row n, amax = max_k |W[n][k]| = m * 2^x with m in [0.5, 1) (frexp):
    e[n] = x - 9 if m <= 0.875 else x - 8      the smallest integer with amax <= 448 * 2^e, clamped to [-126, 127]; 0 for an all-zero row
    scale[n] = 2^e[n]  (fp32)                  q[n][k] = W[n][k] / scale[n] rounded to e4m3fn, nearest-even
So amax / scale lies in (224, 448] for every row whose e is not clamped, and W' = q * scale is exactly a bf16 value.  The row's largest |q|
lies in [224, 448], not in (224, 448]: an amax / scale of 225 .. 232 is nearer to 224 than to 240, the next e4m3 value, and rounds down to it
(about one Gaussian row in fifteen).  Rows whose e is clamped (bf16 subnormals and the smallest normals) have a smaller amax / scale.

The GEMV on byte weights (wg_llama_gemv_e4m3) computes scale[n] * sum_k xh[m][k] q[n][k]: the multiply by a power of two is exact, a lane's
chain is K / 64 long as in the bf16 kernel (16 elements per sweep of 1024), so llm_reference.gemv_reference on the DEQUANTISED weights, bound
unchanged, is its reference.  The two mutants below are wrong weights W'' handed to that reference:
    scale_of_neighbour   row n is scaled by the scale of row n ^ 1 of its segment (the last row of an odd segment by that of the row before)
    cvt_halves_swapped   of every four consecutive bytes, the first two and the last two change places (the two halves of a packed
                         conversion taken in the wrong order)
The test weights give neighbouring rows different magnitudes (2^-3 .. 2^3 by row index), so the first one shows."""
import copy

import torch

from tests import llm_reference as lr

BF16 = lr.BF16
E4M3 = torch.float8_e4m3fn
PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
GEMV_E4M3_MUTANTS = ("scale_of_neighbour", "cvt_halves_swapped")


def row_exponents(w):
    """w [N, K] bf16 -> (e int32 [N], clamped bool [N]) by the frexp rule"""
    amax = w.float().abs().amax(1)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    ec = e.clamp(-126, 127)
    return ec.to(torch.int32), ec != e


def quantize_reference(w):
    """w [N, K] bf16 (CPU) -> (q uint8 [N, K], scale fp32 [N])"""
    assert w.dtype == BF16 and w.dim() == 2
    e, _ = row_exponents(w)
    scale = torch.ldexp(torch.ones(w.shape[0]), e)
    q = (w.float() / scale[:, None]).to(E4M3)
    return q.view(torch.uint8), scale


def dequantize_reference(q, scale):
    """-> W' = q * scale as bf16; the product is formed in fp32 (exact) and must survive the rounding to bf16 unchanged"""
    w = q.view(E4M3).float() * scale[:, None]
    out = w.to(BF16)
    assert out.float().equal(w), "q * scale is not a bf16 value"
    return out


def fake_quantize(w):
    """W' of a bf16 weight on any device, through the CPU reference"""
    return dequantize_reference(*quantize_reference(w.detach().cpu().to(BF16))).to(device=w.device, dtype=w.dtype)


def spread_rows(N, K, seed, std=0.05):
    """Gaussian bf16 rows whose magnitudes differ by row: row n is scaled by 2^((5 n mod 7) - 3), so neighbouring rows never share a scale"""
    w = lr.rand_bf16((N, K), seed, std).float()
    p = (torch.arange(N) * 5) % 7 - 3
    return (w * torch.exp2(p.float())[:, None]).to(BF16)


def special_rows(K):
    """[6, K] bf16: an all-zero row, a row with one outlier, a row whose amax is exactly 448 * 2^-4, one whose amax is the next bf16 above
    that, a row of bf16 subnormals, and a row whose amax / scale is 225 (its largest |q| rounds down to 224)."""
    g = torch.Generator().manual_seed(77)
    base = (torch.randn(6, K, generator=g) * 0.02).to(BF16)
    base[0] = 0
    base[1, K // 3] = 300.0
    edge = torch.tensor([448.0 * 2.0 ** -4], dtype=BF16)
    above = (edge.view(torch.int16) + 1).view(BF16)
    base[2] = base[2].clamp(-1, 1)
    base[2, 5] = -edge[0]
    base[3] = base[3].clamp(-1, 1)
    base[3, K - 1] = above[0]
    sub = torch.randint(1, 128, (K,), generator=g).to(torch.int16)                       # magnitudes 1 .. 127 units of 2^-133
    sub = sub | (torch.randint(0, 2, (K,), generator=g).to(torch.int16) << 15)
    base[4] = sub.view(BF16)
    base[5] = base[5].clamp(-1, 1)
    base[5, 2] = 225.0 * 2.0 ** -6
    return base


def quantiser_case(N, K, seed=5):
    """The weight of the quantiser tests: spread Gaussian rows with special_rows at rows 0 .. 2 and N - 3 .. N - 1"""
    w = spread_rows(N, K, seed)
    sp = special_rows(K)
    w[:3], w[N - 3:] = sp[:3], sp[3:]
    return w


def neighbour(N):
    """row n -> n ^ 1 (the last row of an odd count -> the row before it)"""
    idx = torch.arange(N) ^ 1
    idx[idx >= N] = N - 2
    return idx


def mutant_weights(q, scale, mutant):
    """The wrong W'' [N, K] bf16-valued (as float64) of one segment"""
    assert mutant in GEMV_E4M3_MUTANTS
    v = q.view(E4M3).double()
    if mutant == "scale_of_neighbour":
        return v * scale[neighbour(len(scale))].double()[:, None]
    N, K = v.shape
    v = v.reshape(N, K // 4, 2, 2).flip(2).reshape(N, K)
    return v * scale.double()[:, None]


def gemv_case(M, N, K, nseg, seed=7):
    """x, gamma as test_gpu_llm._gemv_inputs makes them; per segment a spread weight (the odd N gets unequal segments), its bytes, scales and
    W'.  -> x, gamma, [(q, scale)], [W']"""
    x = lr.rand_bf16((M, K), seed, 1.5)
    gamma = lr.rand_bf16((K,), seed + 5, 0.3) + 1
    qs = [quantize_reference(spread_rows(N + (i if N % 2 else 0), K, seed + 1 + i)) for i in range(nseg)]
    return x, gamma, qs, [dequantize_reference(q, s) for q, s in qs]


GEMV_SHAPES = [(M, N, K) for M in (1, 3, 8) for N, K in ((256, 256), (97, 128), (512, 384))] + [(1, 64, 1152), (1, 128, 11008)]
GEMV_OPTS = ["plain1", "plain2", "plain3", "norm", "residual", "pair", "f32", "norm_pair", "norm_f32"]


def gemv_option(M, N, K, opt):
    """One case of the grid, as test_gpu_llm.test_gemv builds its own -> (x, [(q, scale)], [W'], the keywords of gemv_reference, the residual or None)"""
    nseg = {"plain1": 1, "plain2": 2, "plain3": 3, "norm": 3, "residual": 1, "f32": 1, "norm_f32": 1}.get(opt, 2)
    x, gamma, qs, ws = gemv_case(M, N, K, nseg)
    pair = "pair" in opt
    if pair:
        n0 = ws[0].shape[0]
        qs = [qs[0], (qs[1][0][:n0].contiguous(), qs[1][1][:n0].contiguous())]
        ws = [ws[0], ws[1][:n0].contiguous()]
    ntot = ws[0].shape[0] if pair else sum(w.shape[0] for w in ws)
    res = lr.rand_bf16((M, ntot), 19) if opt == "residual" else None
    kw = dict(gamma=gamma if "norm" in opt else None, eps=1e-5, pair=pair, out_f32="f32" in opt)
    return x, qs, ws, kw, res


def dequantized_copy(llm):
    """A deep copy of a LlamaForCausalLM (plain or with lora_reference's adapters) whose seven projection weights per layer are W'"""
    twin = copy.deepcopy(llm)
    with torch.no_grad():
        for layer in twin.model.layers:
            for name in PROJECTIONS:
                owner = layer.self_attn if hasattr(layer.self_attn, name) else layer.mlp
                m = getattr(owner, name)
                m = getattr(m, "base_layer", m)
                m.weight.copy_(fake_quantize(m.weight))
    return twin
