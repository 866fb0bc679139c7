"""CPU-side checks of the LoRA form of the HIP LLaMA path (no GPU): the C-ABI of the two extended entry points, LlamaHipRunner.supports on
adapted models, the references and bounds of tests/lora_reference.py (a CPU emulation of each extended kernel's stated arithmetic lies
inside its bound, every mutant outside it) and the stand-in LoRA layer against the definition."""
import os
import re

import pytest
import torch

from tests import llm_reference as lr
from tests import lora_reference as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LORA_SYMBOLS = ("wg_llama_gemv_lora_bf16", "wg_llama_rope_cache_lora_bf16")


# ---- symbols and argument checks ------------------------------------------------------------------------------------------------------
def test_header_declares_the_lora_entry_points_and_the_version_stays():
    txt = open(os.path.join(ROOT, "include", "walkgpt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in LORA_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert "return 300;" in open(os.path.join(ROOT, "walkgpt_amd", "csrc", "wg_api.hip")).read()
    from walkgpt_amd import _lib
    assert set(LORA_SYMBOLS) <= set(_lib.exported_symbols())


def test_lora_entry_points_reject_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from walkgpt_amd import _lib
    h = _lib.lib()
    assert h.wg_version() == 300
    buf = (torch.zeros(1 << 14, dtype=torch.float32)).data_ptr()    # a 16-byte aligned host address: never dereferenced, the checks come first

    def gemv(x=buf, w1=None, n1=0, pair=0, a0=buf, a1=None, rank=8, t=buf, ldt=24):
        return h.wg_llama_gemv_lora_bf16(x, 128, buf, 4, w1, n1, None, 0, 128, None, 0.0, None, 0, buf, 8, 0, pair, 1, a0, a1, None, rank, t, ldt, None)

    def rope(qkv=buf, bq=buf, bv=None, rank=8, t=buf, ldt=24):
        return h.wg_llama_rope_cache_lora_bf16(qkv, 384, buf, buf, 64, buf, buf, 128, buf, buf, 1, 1, 1, 64, t, ldt, bq, None, bv, 2.0, 0.0, 2.0, rank, None)

    cases = {
        "llama_gemv_lora": [("null x", lambda: gemv(x=None)), ("null t", lambda: gemv(t=None)), ("rank 12", lambda: gemv(rank=12, ldt=36)),
                            ("rank 72", lambda: gemv(rank=72, ldt=216)), ("rank 0", lambda: gemv(rank=0)), ("ldt too small", lambda: gemv(ldt=16)),
                            ("ldt too small at rank 16", lambda: gemv(rank=16, ldt=24)), ("misaligned A", lambda: gemv(a0=buf + 2)),
                            ("misaligned t", lambda: gemv(t=buf + 4)), ("pair mode", lambda: gemv(w1=buf, n1=4, pair=1)),
                            ("adapter on an absent segment", lambda: gemv(a1=buf))],
        "llama_rope_cache_lora": [("null qkv", lambda: rope(qkv=None)), ("null t", lambda: rope(t=None)), ("rank 12", lambda: rope(rank=12, ldt=36)),
                                  ("rank 72", lambda: rope(rank=72, ldt=216)), ("ldt too small", lambda: rope(ldt=16)),
                                  ("misaligned B", lambda: rope(bv=buf + 2)), ("misaligned t", lambda: rope(t=buf + 4))],
    }
    for word, calls in cases.items():
        for what, call in calls:
            rc = call()
            assert rc < 0 and word.encode() in h.wg_last_error(), (word, what, rc, h.wg_last_error())


# ---- supports -------------------------------------------------------------------------------------------------------------------------
def _supports(llm):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    ok, why = LlamaHipRunner.supports(llm)
    assert ok is False
    return why


@pytest.mark.parametrize("targets", [("q_proj", "v_proj"), ("q_proj", "k_proj", "v_proj")])
@pytest.mark.parametrize("r", [8, 16])
def test_supports_takes_unmerged_adapters_on_q_k_v(targets, r):
    """A CPU model is refused for the one thing a CPU model lacks: the adapters themselves qualify."""
    llm = lo.inject_lora(lr.tiny_llm(96), targets, r, 16, 5, 0.06, 0.25)
    assert len(lo.lora_layers(llm)) == 2 * len(targets)
    why = _supports(llm)
    assert "bf16 on a GPU" in why and "merge" not in why, why


def _qv(r=8, **kw):
    return lo.inject_lora(lr.tiny_llm(96), ("q_proj", "v_proj"), r, 16, 5, 0.06, 0.25, **kw)


def _refusals():
    def o_proj():
        return lo.inject_lora(lr.tiny_llm(96), ("q_proj", "o_proj"), 8, 16, 5, 0.06, 0.25)

    def down_proj():
        return lo.inject_lora(lr.tiny_llm(96), ("down_proj",), 8, 16, 5, 0.06, 0.25)

    def rank12():
        return _qv(12)

    def rank72():
        return _qv(72)

    def unequal():
        llm = lo.inject_lora(lr.tiny_llm(96), ("q_proj",), 8, 16, 5, 0.06, 0.25)
        return lo.inject_lora(llm, ("v_proj",), 16, 16, 5, 0.06, 0.25)

    def two_active():
        llm = _qv()
        m = llm.model.layers[1].self_attn.v_proj
        m.add_adapter("second", 8, 16)
        m.active_adapters = ["default", "second"]
        return llm

    def dora():
        llm = _qv()
        llm.model.layers[1].self_attn.q_proj.use_dora["default"] = True
        return llm

    def b_bias():
        llm = _qv()
        a = llm.model.layers[0].self_attn
        a.v_proj = lo.LoraLinear(a.v_proj.base_layer, 8, 16, lora_bias=True)
        return llm

    def dropout():
        llm = _qv()
        a = llm.model.layers[0].self_attn
        a.q_proj = lo.LoraLinear(a.q_proj.base_layer, 8, 16, dropout=0.05)
        return llm.train()

    return [("o_proj", o_proj, "layers.0.self_attn.o_proj", "only q_proj, k_proj and v_proj adapters are built; merge the others"),
            ("down_proj", down_proj, "layers.0.mlp.down_proj", "only q_proj, k_proj and v_proj adapters are built; merge the others"),
            ("rank 12", rank12, "layers.0.self_attn.q_proj", "rank 12"),
            ("rank 72", rank72, "layers.0.self_attn.q_proj", "rank 72"),
            ("unequal ranks", unequal, "layers.0.self_attn.v_proj", "differs"),
            ("two active adapters", two_active, "layers.1.self_attn.v_proj", "2 active adapters"),
            ("DoRA", dora, "layers.1.self_attn.q_proj", "DoRA"),
            ("lora_B bias", b_bias, "layers.0.self_attn.v_proj", "bias"),
            ("dropout in training mode", dropout, "layers.0.self_attn.q_proj", "eval()")]


@pytest.mark.parametrize("what,make,module,word", _refusals(), ids=[c[0] for c in _refusals()])
def test_supports_names_the_module_and_the_cause(what, make, module, word):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    llm = make()
    why = _supports(llm)
    assert module in why and word in why, why
    with pytest.raises(ValueError, match=re.escape(module)):
        LlamaHipRunner(llm)


def test_lora_on_o_proj_has_the_stated_wording():
    llm = lo.inject_lora(lr.tiny_llm(96), ("o_proj",), 8, 16, 5, 0.06, 0.25)
    assert _supports(llm) == "LoRA on layers.0.self_attn.o_proj: only q_proj, k_proj and v_proj adapters are built; merge the others"


@pytest.mark.parametrize("state", ["merged", "disable_adapters"])
def test_merged_or_disabled_layers_count_as_plain(state):
    """also where the adapter itself would be refused: an o_proj adapter, a rank of 12"""
    from walkgpt_amd.llama_hip import LlamaHipRunner
    llm = lo.inject_lora(lr.tiny_llm(96), ("q_proj", "o_proj"), 12, 16, 5, 0.06, 0.25)
    for m in lo.lora_layers(llm):
        setattr(m, state, True)
    assert "bf16 on a GPU" in _supports(llm)
    r = LlamaHipRunner.__new__(LlamaHipRunner)
    r.llm = llm
    assert r._rank() == 0 and all(lw[9] is None for lw in r._layers())
    assert r._layers()[0][1] is llm.model.layers[0].self_attn.q_proj.base_layer.weight          # the module's own tensor, not a copy
    m = lo.lora_layers(llm)[0]
    setattr(m, state, False)
    assert "rank 12" in _supports(llm)


def test_layers_and_weight_key_carry_the_adapters():
    """on a CPU model, through the runner's methods that touch no GPU: the adapter tensors are the modules' own, and the key moves with an
    in-place edit, a scaling and the disabled state"""
    from walkgpt_amd.llama_hip import LlamaHipRunner
    llm = _qv()
    r = LlamaHipRunner.__new__(LlamaHipRunner)
    r.llm = llm
    q = llm.model.layers[1].self_attn.q_proj
    lora = r._layers()[1][9]
    assert r._rank() == 8 and lora[1] is None and lora[0][0] == "default" and lora[0][3] == 2.0
    assert lora[0][1] is q.lora_A["default"].weight and lora[0][2] is q.lora_B["default"].weight
    keys = [r._weight_key()]
    assert r._weight_key() == keys[0]
    with torch.no_grad():
        q.lora_B["default"].weight.mul_(4.0)
    keys.append(r._weight_key())
    with torch.no_grad():
        q.lora_A["default"].weight.mul_(1.0)
    keys.append(r._weight_key())
    q.scaling["default"] = 1.0
    keys.append(r._weight_key())
    q.disable_adapters = True
    keys.append(r._weight_key())
    assert len(set(keys)) == len(keys)


# ---- emulations inside the bounds, mutants outside ------------------------------------------------------------------------------------
def _worst(got, ref_bound):
    ref, bound = ref_bound
    if bound is None:
        return 0.0 if got.equal(ref) else float("inf")
    return lr.bound_check(got, ref, bound)[0]


@pytest.mark.parametrize("past,L", [(0, 1), (70, 65)])
@pytest.mark.parametrize("r", [8, 16])
@pytest.mark.parametrize("adapted", ["qv", "qkv"])
def test_rope_lora_emulation_inside_mutants_outside(past, L, r, adapted):
    qkv, t, lora_b, scales = lo.rope_lora_inputs(2, L, 2, r, adapted)
    pos = past + torch.arange(L)
    refs = lo.rope_lora_reference(qkv, pos, t, lora_b, scales, 2)
    emu = lo.rope_lora_reference(qkv, pos, t, lora_b, scales, 2, emulate=True)
    worst = [_worst(e[0], rb) for e, rb in zip(emu, refs)]
    print("rope lora emulation past %d L %d r %d %s: worst %s of the bound (q, k, v)" % (past, L, r, adapted, ["%.3f" % w for w in worst]))
    assert max(worst) <= 1.0
    for mutant in lo.ROPE_LORA_MUTANTS:
        if mutant == "delta_after_rotation" and past + L == 1:
            continue                                                 # (position 0 alone: the rotation is the identity, the order cannot show)
        if mutant == "b_row_stride" and r == 8:
            continue                                                 # (a row stride of 8 is the right one at r = 8)
        bad = lo.rope_lora_reference(qkv, pos, t, lora_b, scales, 2, mutant=mutant)
        w = [_worst(b[0], rb) for b, rb in zip(bad, refs)]
        print("  mutant %s: %s x the bound (q, k, v)" % (mutant, ["%.1f" % x for x in w]))
        assert max(w) > 1.0, mutant
        if mutant == "adapters_swapped":
            assert w[0] > 1.0 and w[2] > 1.0
        if mutant == "delta_after_rotation":
            assert w[0] > 1.0


def test_rope_lora_reference_without_adapters_is_the_plain_reference():
    qkv, t, _, scales = lo.rope_lora_inputs(2, 5, 2, 8, "")
    pos = 3 + torch.arange(5)
    q, k, v = lo.rope_lora_reference(qkv, pos, t, [None] * 3, scales, 2)
    for got, x in ((q, qkv[..., :256]), (k, qkv[..., 256:512])):
        ref, bound = lr.rope_reference(x, pos)
        assert got[0].equal(ref) and got[1].equal(bound)
    assert v[1] is None and v[0].equal(qkv[..., 512:].double())


def _gemv(M, N, K, r, adapted):
    x = lr.rand_bf16((M, K), 7, 1.5)
    ws = [lr.rand_bf16((N + (i if N % 2 else 0), K), 8 + i, 0.05) for i in range(3)]
    lora_a = [lr.rand_bf16((r, K), 30 + i, 0.06) if ch in adapted else None for i, ch in enumerate("qkv")]
    return x, ws, lora_a, lr.rand_bf16((K,), 12, 0.3) + 1


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("M,N,K,r,adapted", [(3, 97, 128, 8, "qv"), (8, 64, 384, 16, "qkv"), (1, 32, 4096, 8, "v")])
def test_gemv_lora_emulation_inside_mutant_outside(norm, M, N, K, r, adapted):
    x, ws, lora_a, gamma = _gemv(M, N, K, r, adapted)
    kw = dict(gamma=gamma if norm else None, eps=1e-5)
    ref, bound, t_ref, t_bound, cols = lo.gemv_lora_reference(x, ws, lora_a, **kw)
    emu, _, t_emu, _, _ = lo.gemv_lora_reference(x, ws, lora_a, emulate=True, **kw)
    w_out, w_t = lr.bound_check(emu, ref, bound)[0], lr.bound_check(t_emu[:, cols], t_ref[:, cols], t_bound[:, cols])[0]
    print("gemv lora emulation M %d N %d K %d r %d %s norm %s: out %.3f, t %.3f of the bound" % (M, N, K, r, adapted, norm, w_out, w_t))
    assert w_out <= 1.0 and w_t <= 1.0 and len(cols) == r * len(adapted)
    if norm:
        _, _, t_bad, _, _ = lo.gemv_lora_reference(x, ws, lora_a, mutant="a_rows_unnormed", **kw)
        w = lr.bound_check(t_bad[:, cols], t_ref[:, cols], t_bound[:, cols])[0]
        print("  mutant a_rows_unnormed: %.1f x the bound" % w)
        assert w > 1.0


# ---- the stand-in against the definition ----------------------------------------------------------------------------------------------
def test_stand_in_forward_is_the_merged_weight():
    torch.manual_seed(0)
    base = torch.nn.Linear(96, 40, bias=False)
    m = lo.LoraLinear(base, 8, 16)
    with torch.no_grad():
        m.lora_B["default"].weight.normal_(0, 0.3)
    x = torch.randn(5, 96)
    W = base.weight + m.scaling["default"] * m.lora_B["default"].weight @ m.lora_A["default"].weight
    want = x @ W.T
    with torch.no_grad():
        got = m(x)
        assert float((got - want).norm() / want.norm()) <= 1e-5
        assert not torch.allclose(got, base(x), rtol=1e-2, atol=0)
        for state in ("merged", "disable_adapters"):
            setattr(m, state, True)
            assert m(x).equal(base(x))
            setattr(m, state, False)
    assert m.scaling["default"] == 2.0 and m.use_dora == {"default": False} and m.active_adapters == ["default"]
