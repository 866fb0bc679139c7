"""Unmerged LoRA adapters on the HIP LLaMA path (plain module, shared by tests/test_lora_host.py and tests/test_gpu_lora.py): a stand-in for
peft.tuners.lora.layer.Linear (peft is not needed), `inject_lora`, and float64 references with derived per-element bounds for the two
extended kernels of walkgpt_amd/csrc/llama.hip, in the manner of tests/llm_reference.py (u = 2^-24, the bf16 unit roundoff 2^-8).

GEMV with adapter rows (wg_llama_gemv_lora_bf16).  The rows of A_i are further weight rows of the launch: they see the same unrounded
xh = x * rstd * gamma as the W rows, are summed the same way and leave as fp32.  So the bf16 outputs keep llm_reference.gemv_reference's
bound (and are the plain kernel's bits), and t[m][i r + j] = A_i[j] . xh[m] has gemv_reference's bound for an fp32 output,
    2^-24 |ref| + (K / 64 + K / 256 + 32) u sum_k |xh_k A_jk|.

RoPE + cache with the up-projection (wg_llama_rope_cache_lora_bf16).  The kernel states, for an adapted projection and t as given:
    d  = s * sum_j B[n][j] t[j]       fp32, j ascending, r terms         x' = x[n] + d      fp32, x the bf16 value of W xh
    q, k = bf16(rope(x'))             the rotation as today              v  = bf16(x')
With D = |s| sum_j |B[n][j] t[j]| and X = |x| + D (>= |x'|):
    the sum            r products (u each; B is bf16, exact in fp32) and r - 1 additions: <= r u D in any order of the terms (fast-math may
                       reorder, an fma only drops roundings); times s: + u D
    x + d              u |x'| <= u X                                    so x' carries at most (r + 2) u X, taken as (r + 3) u X
    v                  one rounding: 2^-8 |ref| + (r + 3) u X, taken as 2^-8 |ref| + (r + 4) u X
    q, k               out = bf16(a' c -/+ b' s): today's 2^-8 |ref| + 4 u (|a' c| + |b' s|) (tables within 2 u of the float64 cos / sin of the
                       SAME fp32 angle, a product, the subtraction), with |a'| <= X_a, |b'| <= X_b, plus what a' and b' carry, times
                       |c|, |s|: together (r + 7) u (X_a |c| + X_b |s|), taken as
                       2^-8 |ref| + (r + 8) u (X_a |c| + X_b |s|)
    An unadapted q / k keeps llm_reference.rope_reference's bound, an unadapted v is a copy: exact.
t is taken as given: its own error is bounded by the GEMV test.

`emulate=` computes what a faithful kernel computes (fp32, the stated roundings), `mutant=` gives deliberately wrong results;
tests/test_lora_host.py holds every emulation inside its bound and every mutant outside it, on the CPU."""
import torch
from torch import nn

from tests import llm_reference as lr

U32, UBF, BF16 = lr.U32, lr.UBF, lr.BF16
TARGETS = ("q_proj", "k_proj", "v_proj")
ALL_PROJECTIONS = TARGETS + ("o_proj", "gate_proj", "up_proj", "down_proj")


# ---- the stand-in layer ---------------------------------------------------------------------------------------------------------------
class LoraLinear(nn.Module):
    """The attributes and the forward of peft.tuners.lora.layer.Linear with one adapter (further ones: add_adapter).  It rounds in the
    weights' dtype, as nn.Linear does."""

    def __init__(self, base, r, alpha, name="default", dropout=0.0, lora_bias=False):
        super().__init__()
        self.base_layer = base
        self.lora_A, self.lora_B, self.lora_dropout = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        self.scaling, self.use_dora = {}, {}
        self.active_adapters = [name]
        self.merged = False
        self.disable_adapters = False
        self.add_adapter(name, r, alpha, dropout, lora_bias)

    def add_adapter(self, name, r, alpha, dropout=0.0, lora_bias=False):
        w = self.base_layer.weight
        kw = dict(device=w.device, dtype=w.dtype)
        self.lora_A[name] = nn.Linear(self.base_layer.in_features, r, bias=False, **kw)
        self.lora_B[name] = nn.Linear(r, self.base_layer.out_features, bias=lora_bias, **kw)
        self.lora_dropout[name] = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.scaling[name] = alpha / r
        self.use_dora[name] = False

    def forward(self, x):
        out = self.base_layer(x)
        if self.merged or self.disable_adapters:
            return out
        for a in self.active_adapters:
            if a in self.lora_A:
                out = out + self.lora_B[a](self.lora_A[a](self.lora_dropout[a](x))) * self.scaling[a]
        return out


def lora_layers(llm):
    return [m for m in llm.modules() if isinstance(m, LoraLinear)]


def inject_lora(llm, targets, r, alpha, seed, std_a, std_b):
    """Replace the projections named in `targets` (of self_attn or mlp) in every layer by a LoraLinear around them, in place.  A ~ N(0, std_a),
    B ~ N(0, std_b) (std_b: one figure or a dict per target), drawn on the CPU from (seed, layer, target) and rounded to bf16, kept in the
    model's dtype: the same seed gives the same adapters in a bf16 model and in its fp32 twin."""
    for i, layer in enumerate(llm.model.layers):
        for tname in targets:
            owner = layer.self_attn if hasattr(layer.self_attn, tname) else layer.mlp
            base = getattr(owner, tname)
            m = LoraLinear(base, r, alpha)
            g = torch.Generator().manual_seed(seed * 1000003 + i * 101 + ALL_PROJECTIONS.index(tname))
            sb = std_b[tname] if isinstance(std_b, dict) else std_b
            a = (torch.randn(r, base.in_features, generator=g) * std_a).to(BF16)
            b = (torch.randn(base.out_features, r, generator=g) * sb).to(BF16)
            with torch.no_grad():
                m.lora_A["default"].weight.copy_(a)
                m.lora_B["default"].weight.copy_(b)
            m.train(llm.training)
            setattr(owner, tname, m)
    return llm


# ---- GEMV with adapter rows -------------------------------------------------------------------------------------------------------------
GEMV_LORA_MUTANTS = ("a_rows_unnormed",)


def gemv_lora_reference(x, weights, lora_a, gamma=None, eps=0.0, mutant=None, emulate=False):
    """x [M, K] bf16, weights one to three [N_i, K] bf16, lora_a per weight an [r, K] bf16 or None.
    -> (ref, bound, t_ref, t_bound, cols): ref / bound [M, sum N_i] as lr.gemv_reference's; t_ref / t_bound [M, 3 r] float64 and `cols`, the
    columns of t that an adapter owns (the others hold 0 / infinity here and are left alone by the kernel)."""
    assert mutant is None or mutant in GEMV_LORA_MUTANTS
    ref, bound = lr.gemv_reference(x, weights, gamma=gamma, eps=eps, emulate=emulate)
    lora_a = list(lora_a) + [None] * (3 - len(lora_a))
    r = next(a.shape[0] for a in lora_a if a is not None)
    M = x.shape[0]
    t_ref = torch.zeros(M, 3 * r, dtype=torch.float64)
    t_bound = torch.full((M, 3 * r), float("inf"), dtype=torch.float64)
    cols = []
    for i, a in enumerate(lora_a):
        if a is None:
            continue
        g = None if mutant == "a_rows_unnormed" else gamma
        tr, _ = lr.gemv_reference(x, [a], gamma=g, eps=eps, out_f32=True, emulate=emulate)
        _, tb = lr.gemv_reference(x, [a], gamma=gamma, eps=eps, out_f32=True)
        t_ref[:, i * r:(i + 1) * r], t_bound[:, i * r:(i + 1) * r] = tr, tb
        cols += list(range(i * r, (i + 1) * r))
    return ref, bound, t_ref, t_bound, torch.tensor(cols)


# ---- RoPE + cache with the up-projection ------------------------------------------------------------------------------------------------
ROPE_LORA_MUTANTS = ("scaling_dropped", "delta_after_rotation", "adapters_swapped", "b_row_stride")


def _rot(xv, c, s):
    a, b = xv[..., :64], xv[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def rope_lora_reference(qkv, positions, t, lora_b, scales, heads, theta=10000.0, emulate=False, mutant=None):
    """qkv [rows, L, 3H] bf16 (q | k | v), positions [L], t [rows, L, 3 r] fp32 (taken as given), lora_b = (B_q, B_k, B_v) each [H, r] bf16 or
    None, scales their three scalings.  -> [(ref, bound)] * 3 for q, k, v, float64 [rows, L, H]; the bound of an unadapted v is None: a copy."""
    assert mutant is None or mutant in ROPE_LORA_MUTANTS
    rows, L, H3 = qkv.shape
    H = H3 // 3
    r = t.shape[-1] // 3
    dt = torch.float32 if emulate else torch.float64
    inv_freq = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    ang = (positions.float()[:, None] * inv_freq[None, :]).double()                    # [L, 64], the fp32 angle
    c, s = ang.cos().to(dt)[:, None, :], ang.sin().to(dt)[:, None, :]
    heads_of = lambda v: v.reshape(rows, L, heads, 128)

    def delta(seg):
        """-> (d, D) of the adapter that acts on projection `seg`: s B t and |s| |B| |t|, [rows, L, H]; None without one"""
        src = {0: 2, 2: 0}.get(seg, seg) if mutant == "adapters_swapped" else seg
        if lora_b[src] is None:
            return None
        B, ts = lora_b[src].to(dt), t[..., src * r:(src + 1) * r].to(dt)
        if mutant == "b_row_stride":                                                    # row n read at n * 8, not n * r
            flat = torch.cat([B.reshape(-1), B.new_zeros(r)])
            B = flat[(torch.arange(H)[:, None] * 8 + torch.arange(r)[None, :])]
        sc = 1.0 if mutant == "scaling_dropped" else float(scales[src])
        return sc * (ts @ B.T), abs(sc) * (ts.abs() @ B.abs().T)

    out = []
    for seg in range(3):
        x = qkv[..., seg * H:(seg + 1) * H].to(dt)
        dd = delta(seg)
        if dd is None:
            if seg < 2:
                out.append(lr.rope_reference(qkv[..., seg * H:(seg + 1) * H], positions, theta, emulate=emulate))
            else:
                out.append((x.double(), None))
            continue
        d, D = dd
        X = x.abs() + D
        if seg == 2:
            ref = x + d
            bound = UBF * ref.abs() + (r + 4) * U32 * X + 1e-30
        else:
            if mutant == "delta_after_rotation":
                ref = _rot(heads_of(x), c, s).reshape(rows, L, H) + d
            else:
                ref = _rot(heads_of(x + d), c, s).reshape(rows, L, H)
            Xh = heads_of(X)
            mag = torch.cat([Xh[..., :64] * c.abs() + Xh[..., 64:] * s.abs(), Xh[..., 64:] * c.abs() + Xh[..., :64] * s.abs()], -1).reshape(rows, L, H)
            bound = UBF * ref.abs() + (r + 8) * U32 * mag + 1e-30
        if emulate:
            ref = ref.to(BF16)
        out.append((ref.double(), bound.double()))
    return out


def rope_lora_inputs(rows, L, heads, r, adapted, seed=3):
    """The inputs of the rope tests: qkv ~ N(0, 1) as test_rope_cache's, t ~ N(0, 1) fp32, B ~ N(0, 0.25) for the projections named in
    `adapted` (a subset of "qkv"), scalings 2, 0.5 and 1.5: the adapter's term is of the size of the value it is added to."""
    H = heads * 128
    qkv = lr.rand_bf16((rows * L, 3 * H), seed).reshape(rows, L, 3 * H)
    g = torch.Generator().manual_seed(seed + 100)
    t = torch.randn(rows, L, 3 * r, generator=g)
    lora_b = [lr.rand_bf16((H, r), seed + 200 + i, 0.25) if ch in adapted else None for i, ch in enumerate("qkv")]
    return qkv, t, lora_b, (2.0, 0.5, 1.5)
