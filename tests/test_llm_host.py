"""CPU-side checks of the HIP LLaMA path (no GPU): the C-ABI of csrc/llama.hip, the public switch, LlamaHipRunner.supports, the host RoPE
table, the references and bounds of tests/llm_reference.py (a CPU emulation of each kernel's stated arithmetic lies inside its bound, every
mutant outside it), and the host's stop rule against walkgptForCausalLM._generate."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from tests import attn_reference as ar
from tests import llm_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wg_rmsnorm_rows_bf16", "wg_llama_rope_cache_bf16", "wg_llama_attn_prefill_bf16", "wg_llama_attn_decode_bf16",
               "wg_llama_attn_decode_workspace_floats", "wg_llama_gemv_bf16", "wg_llama_silu_mul_bf16", "wg_llama_pick_token")


# ---- symbols and the switch -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_llama_entry_points_and_the_version_stays():
    txt = open(os.path.join(ROOT, "include", "walkgpt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    assert "return 300;" in open(os.path.join(ROOT, "walkgpt_amd", "csrc", "wg_api.hip")).read()
    from walkgpt_amd import _lib
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())


def test_switch_exists_and_is_off_by_default():
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    assert walkgptForCausalLM._hip_llm is None and callable(walkgptForCausalLM.enable_hip_llm)
    m = walkgptForCausalLM.__new__(walkgptForCausalLM)
    nn.Module.__init__(m)
    assert m.hip_llm_enabled is False
    m.llm = lr.tiny_llm(96, dtype=torch.float32)                    # a CPU fp32 model does not qualify: the switch raises with the reason
    with pytest.raises(ValueError, match="bf16 on a GPU"):
        m.enable_hip_llm()
    assert m.hip_llm_enabled is False and m.enable_hip_llm(False) is m


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from walkgpt_amd import _lib
    h = _lib.lib()
    assert h.wg_version() == 300
    buf = (torch.zeros(1 << 14, dtype=torch.float32)).data_ptr()    # a 16-byte aligned host address: never dereferenced, the checks come first
    cases = {
        "rmsnorm": [lambda: h.wg_rmsnorm_rows_bf16(None, 8, None, None, 8, 1, 8, 1e-5, None, 0, 0, 0, None),
                    lambda: h.wg_rmsnorm_rows_bf16(buf, 12, buf, buf, 12, 1, 12, 1e-5, None, 0, 0, 0, None),
                    lambda: h.wg_rmsnorm_rows_bf16(buf, 8, buf, buf, 8, 1, 8, 1e-5, buf, 0, 0, 0, None)],
        "llama_rope_cache": [lambda: h.wg_llama_rope_cache_bf16(None, 0, None, None, 0, None, None, 0, None, None, 1, 1, 1, 64, None),
                             lambda: h.wg_llama_rope_cache_bf16(buf, 384, buf, buf, 64, buf, buf, 128, buf, buf, 1, 1, 1, 100, None),
                             lambda: h.wg_llama_rope_cache_bf16(buf, 128, buf, buf, 64, buf, buf, 128, buf, buf, 1, 1, 1, 64, None)],
        "llama_attn_prefill": [lambda: h.wg_llama_attn_prefill_bf16(None, 0, None, None, None, None, 0, None, 1, 1, 1, 64, 1.0, None),
                               lambda: h.wg_llama_attn_prefill_bf16(buf, 128, buf, buf, buf, buf, 128, buf, 1, 65, 1, 64, 1.0, None),
                               lambda: h.wg_llama_attn_prefill_bf16(buf, 128, buf, buf, buf, buf, 128, buf, 1, 1, 1, 96, 1.0, None)],
        "llama_attn_decode": [lambda: h.wg_llama_attn_decode_bf16(None, 0, None, None, None, None, 0, None, 0, None, 1, 1, 64, 1.0, None),
                              lambda: h.wg_llama_attn_decode_bf16(buf, 128, buf, buf, buf, buf, 8, buf, 128, buf, 1, 1, 64, 1.0, None),
                              lambda: h.wg_llama_attn_decode_bf16(buf, 128, buf, buf, buf, buf, 1 << 20, buf, 128, buf, 1, 1, 65, 1.0, None)],
        "llama_gemv": [lambda: h.wg_llama_gemv_bf16(None, 0, None, 0, None, 0, None, 0, 128, None, 0.0, None, 0, None, 0, 0, 0, 1, None),
                       lambda: h.wg_llama_gemv_bf16(buf, 128, buf, 4, None, 0, None, 0, 128, None, 0.0, None, 0, buf, 4, 0, 0, 9, None),
                       lambda: h.wg_llama_gemv_bf16(buf, 192, buf, 4, None, 0, None, 0, 192, None, 0.0, None, 0, buf, 4, 0, 0, 1, None),
                       lambda: h.wg_llama_gemv_bf16(buf, 128, buf, 4, buf, 5, None, 0, 128, None, 0.0, None, 0, buf, 4, 0, 1, 1, None),
                       lambda: h.wg_llama_gemv_bf16(buf, 128, buf, 4, None, 0, None, 0, 128, None, 0.0, None, 0, buf, 3, 0, 0, 1, None)],
        "llama_silu_mul": [lambda: h.wg_llama_silu_mul_bf16(None, 0, None, 0, 1, 8, None),
                           lambda: h.wg_llama_silu_mul_bf16(buf, 16, buf, 8, 1, 12, None)],
        "llama_pick_token": [lambda: h.wg_llama_pick_token(None, 0, None, 0, None, 0, None, 0, None, None, None, -1, 0, 1, 1, 8, 64, None),
                             lambda: h.wg_llama_pick_token(buf, 96, buf, 96, buf, 256, buf, 4, buf, buf, buf, -1, 0, 9, 96, 256, 64, None),
                             lambda: h.wg_llama_pick_token(buf, 96, buf, 96, buf, 256, buf, 4, buf, buf, buf, 2, 200, 1, 96, 256, 64, None),
                             lambda: h.wg_llama_pick_token(buf, 96, buf, 96, buf, 256, buf, 4, buf, buf, buf, -1, 0, 1, 96, 256, 60, None)],
    }
    for word, calls in cases.items():
        for i, call in enumerate(calls):
            rc = call()
            assert rc < 0 and word.encode() in h.wg_last_error(), (word, i, rc, h.wg_last_error())
    assert h.wg_llama_attn_decode_workspace_floats(2, 32) >= 2 * 32 * 130 and h.wg_llama_attn_decode_workspace_floats(0, 32) == 0


# ---- supports -------------------------------------------------------------------------------------------------------------------------
class _Wrapped(nn.Module):
    """what a PEFT / LoRA layer looks like from outside: a module that holds the Linear"""

    def __init__(self, base):
        super().__init__()
        self.base_layer = base

    def forward(self, x):
        return self.base_layer(x)


@pytest.mark.parametrize("what,over,word", [
    ("gqa", dict(num_key_value_heads=1), "grouped-query"),
    ("head_dim 64", dict(num_attention_heads=4, num_key_value_heads=4), "head_dim 64"),
    ("rope scaling", dict(rope_scaling={"rope_type": "linear", "factor": 2.0}), "rope scaling"),
    ("mlp bias", dict(mlp_bias=True), "bias"),
    ("fp32", dict(), "bf16 on a GPU"),
    ("wrapper", dict(), "merge the adapters first"),
])
def test_supports_says_why_not(what, over, word):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    llm = lr.tiny_llm(96, dtype=torch.float32 if what == "fp32" else torch.bfloat16, **over)
    if what == "wrapper":
        llm.model.layers[1].self_attn.v_proj = _Wrapped(llm.model.layers[1].self_attn.v_proj)
    ok, why = LlamaHipRunner.supports(llm)
    assert ok is False and word in why, why
    with pytest.raises(ValueError):
        LlamaHipRunner(llm)


# ---- RoPE table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [10000.0, 500000.0])
def test_rope_table_equals_llama_rotary_embedding(theta):
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    from walkgpt_amd.llama_hip import rope_table
    cfg = lr.tiny_config(96, rope_theta=theta)
    if getattr(cfg, "rope_parameters", None):
        cfg.rope_parameters["rope_theta"] = theta
    cos, sin = rope_table(cfg, 601)
    rc, rs = LlamaRotaryEmbedding(cfg)(torch.zeros(1, 1, dtype=torch.float32), torch.arange(601)[None])
    assert rc.dtype == torch.float32 and rc.shape == (1, 601, 128)
    assert float((rc[0, :, :64] - cos).abs().max()) <= 1e-6 and float((rs[0, :, :64] - sin).abs().max()) <= 1e-6
    assert rc[0, :, 64:].equal(rc[0, :, :64])                       # the two halves are equal: 64 columns hold all of it
    assert float((cos[600] - torch.cos(600 * theta ** (-torch.arange(0, 128, 2).double() / 128))).abs().max()) < 1e-4


# ---- emulations inside the bounds, mutants outside ------------------------------------------------------------------------------------
def _attn(L, past):
    q = ar.rand_bf16((2, L, 256), 40, 3.0)
    k, v = ar.rand_bf16((2, past + L, 256), 41), ar.rand_bf16((2, past + L, 256), 42)
    return q, k, v, lr.attn_mask_rows(2, past + L)


@pytest.mark.parametrize("L,past", [(1, 0), (1, 200), (65, 0), (130, 40)])
def test_attention_emulation_inside_mutants_outside(L, past):
    q, k, v, mask = _attn(L, past)
    ref, A = lr.attn_reference(q, k, v, 2, mask, past)
    emu, _ = lr.attn_reference(q, k, v, 2, mask, past, emulate=True)
    worst, _ = ar.check(emu, ref, A)
    print("attention emulation L %d past %d: worst %.3f of the bound" % (L, past, worst))
    assert worst <= 1.0
    if past + L > 20:
        for mutant in lr.ATTN_MUTANTS:
            if mutant == "causal_off_by_one" and L == 1:
                continue                                             # (one query at the last position: nothing lies behind it)
            bad, _ = lr.attn_reference(q, k, v, 2, mask, past, mutant=mutant)
            w, _ = ar.check(bad, ref, A)
            print("  mutant %s: %.1f x the bound" % (mutant, w))
            assert w > 1.0, mutant


def _gemv(M, N, K, nseg, x_std=1.5):
    x = lr.rand_bf16((M, K), 7, x_std)
    ws = [lr.rand_bf16((N, K), 8 + i, 0.05) for i in range(nseg)]
    return x, ws, lr.rand_bf16((K,), 12, 0.3) + 1, lr.rand_bf16((M, N * nseg), 19)


@pytest.mark.parametrize("opt", ["plain", "norm", "residual", "pair", "f32", "norm_pair"])
@pytest.mark.parametrize("M,N,K", [(3, 97, 128), (8, 64, 384), (1, 32, 11008)])
def test_gemv_emulation_inside_the_bound(opt, M, N, K):
    x, ws, gamma, res = _gemv(M, N, K, 2)
    kw = dict(gamma=gamma if "norm" in opt else None, eps=1e-5, pair="pair" in opt, out_f32=opt == "f32", residual=res if opt == "residual" else None)
    ref, bound = lr.gemv_reference(x, ws, **kw)
    emu, _ = lr.gemv_reference(x, ws, emulate=True, **kw)
    worst, _ = lr.bound_check(emu, ref, bound)
    print("gemv emulation %s M %d N %d K %d: worst %.3f of the bound" % (opt, M, N, K, worst))
    assert worst <= 1.0


def test_gemv_mutants_outside_the_bound():
    x, ws, gamma, _ = _gemv(3, 64, 384, 2)
    for kw, mutant in ((dict(), "drop_k_block"), (dict(gamma=gamma, eps=1e-5), "drop_k_block"), (dict(pair=True), "gate_up_swapped"),
                       (dict(pair=True, gamma=gamma, eps=1e-5), "gate_up_swapped")):
        ref, bound = lr.gemv_reference(x, ws, **kw)
        bad, _ = lr.gemv_reference(x, ws, mutant=mutant, **kw)
        w, _ = lr.bound_check(bad, ref, bound)
        print("gemv mutant %s %s: %.1f x the bound" % (mutant, sorted(kw), w))
        assert w > 1.0
    # eps outside the square root moves rstd by eps / (2 rms) relatively: it shows where the row is small against sqrt(eps) -- a row of
    # rms 0.004 against eps 1e-5 -- and is far below a bf16 rounding on rows of rms ~ 1, so this mutant is run on the small row
    xs = lr.rand_bf16((3, 384), 7, 0.004)
    for out_f32 in (False, True):
        ref, bound = lr.gemv_reference(xs, ws, gamma=gamma, eps=1e-5, out_f32=out_f32)
        bad, _ = lr.gemv_reference(xs, ws, gamma=gamma, eps=1e-5, out_f32=out_f32, mutant="eps_outside_sqrt")
        emu, _ = lr.gemv_reference(xs, ws, gamma=gamma, eps=1e-5, out_f32=out_f32, emulate=True)
        w, we = lr.bound_check(bad, ref, bound)[0], lr.bound_check(emu, ref, bound)[0]
        print("gemv mutant eps_outside_sqrt (fp32 out %s): %.1f x the bound (the emulation: %.3f)" % (out_f32, w, we))
        assert w > 1.0 and we <= 1.0


@pytest.mark.parametrize("D", [256, 4096])
def test_rmsnorm_emulation_inside_the_bound(D):
    x, w = lr.rand_bf16((3, D), 1, 2.0), lr.rand_bf16((D,), 2) + 1
    ref, bound = lr.rmsnorm_reference(x, w, 1e-5)
    emu, _ = lr.rmsnorm_reference(x, w, 1e-5, emulate=True)
    assert lr.bound_check(emu, ref, bound)[0] <= 1.0
    assert lr.bound_check(ref * (1 + 2.0 ** -6), ref, bound)[0] > 1.0


def test_rope_emulation_inside_and_the_interleaved_pairing_outside():
    x = lr.rand_bf16((2, 65, 256), 3)
    pos = 70 + torch.arange(65)
    ref, bound = lr.rope_reference(x, pos)
    emu, _ = lr.rope_reference(x, pos, emulate=True)
    bad, _ = lr.rope_reference(x, pos, pairing="interleaved")
    w_emu, w_bad = lr.bound_check(emu, ref, bound)[0], lr.bound_check(bad, ref, bound)[0]
    print("rope emulation %.3f of the bound; the (2i, 2i + 1) pairing %.1f x" % (w_emu, w_bad))
    assert w_emu <= 1.0 and w_bad > 1.0
    # transformers' own apply_rotary_pos_emb, in float64 on the same angles, is the reference's pairing
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    ang = (pos.float()[:, None] * inv_freq[None, :]).double()
    emb = torch.cat([ang, ang], -1)[None]
    xq = x.double().reshape(2, 65, 2, 128).transpose(1, 2)
    hf, _ = apply_rotary_pos_emb(xq, xq, emb.cos(), emb.sin())
    assert float((hf.transpose(1, 2).reshape(2, 65, 256) - ref).abs().max()) < 1e-12


# ---- the host's stop rule against _generate -----------------------------------------------------------------------------------------------
class _ScriptedLM:
    """`self.llm` of _generate: emits script[row][step] as the argmax of step `step`; the cache is just the number of positions seen"""

    def __init__(self, script, L0, V=16, H=8):
        self.script, self.L0, self.V = script, L0, V
        self.table = torch.randn(V, H, generator=torch.Generator().manual_seed(0))

    def get_input_embeddings(self):
        return SimpleNamespace(weight=self.table)

    def __call__(self, inputs_embeds=None, attention_mask=None, past_key_values=None, **kw):
        rows, n, H = inputs_embeds.shape
        seen = (past_key_values or 0) + n
        assert attention_mask.shape == (rows, seen)
        step = seen - self.L0
        logits = torch.zeros(rows, n, self.V)
        for r in range(rows):
            logits[r, -1, self.script[r][step]] = 5.0
        return SimpleNamespace(logits=logits, hidden_states=(inputs_embeds.clone(),), past_key_values=seen)


@pytest.mark.parametrize("name,script,eos,pad,max_new", [
    ("eos in different steps", [[3, 4, 9, 5, 6, 7, 8, 3], [3, 4, 5, 6, 7, 9, 8, 3]], 9, 1, 8),
    ("eos in the first step", [[9, 4, 5, 6], [9, 4, 5, 6]], 9, 1, 4),
    ("one row never finishes", [[3, 9, 5, 6, 7, 8], [3, 4, 5, 6, 7, 8]], 9, 1, 6),
    ("eos None", [[3, 9, 5, 6, 7], [9, 4, 9, 6, 7]], None, 1, 5),
    ("pad None", [[3, 9, 5, 6, 7, 8], [3, 4, 5, 9, 7, 8]], 9, None, 6),
    ("the last step", [[3, 4, 5, 9], [3, 4, 5, 9]], 9, 1, 4),
])
def test_stop_rule_matches_generate(name, script, eos, pad, max_new):
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    from walkgpt_amd.llama_hip import trimmed_length
    L0, rows = 5, len(script)
    lm = _ScriptedLM(script, L0)
    fake = SimpleNamespace(llm=lm, eos_token_id=eos, config=SimpleNamespace(pad_token_id=pad), _hip_llm=None)
    embeds = torch.zeros(rows, L0, 8)
    want, hidden = walkgptForCausalLM._generate(fake, embeds, torch.ones(rows, L0, dtype=torch.bool), max_new)
    # what the device writes: the pick rule applied at EVERY step (the device does not stop), then the host trims
    pad_eff = eos if pad is None else pad
    fin, raw = [False] * rows, []
    for step in range(max_new):
        logits = torch.zeros(rows, lm.V)
        for r in range(rows):
            logits[r, script[r][step]] = 5.0
        raw.append(lr.pick_reference(logits, fin, eos, pad_eff))
    raw = torch.tensor(raw).T
    for sync_every in (1, 3, 8):
        done, n = 1, None
        while n is None:
            n = trimmed_length(raw[:, :done], eos, max_new)
            if n is None:
                done = min(done + sync_every, max_new)
        assert n == want.shape[1] and raw[:, :n].equal(want), (name, sync_every, n, want)
        assert hidden.shape[1] == L0 + n - 1
