"""CPU-side checks of the e4m3 weight-only mode of the HIP LLaMA path (no GPU): the quantisation format's properties on the torch reference
of tests/fp8w_reference.py, the GEMV mutants of this mode against llm_reference.gemv_reference's unchanged bound at every shape the GPU test
runs, the C-ABI of the new entry points, the `weights=` validation and the byte store's key behaviour."""
import os
import re

import pytest
import torch
from torch import nn

from tests import fp8w_reference as fr
from tests import llm_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
NEW_SYMBOLS = ("wg_llama_quantize_weight_e4m3", "wg_llama_dequantize_weight_bf16", "wg_llama_gemv_e4m3", "wg_llama_gemv_lora_e4m3")


# ---- the format -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(97, 128), (256, 384)])
def test_reference_quantiser_properties(N, K):
    w = fr.quantiser_case(N, K)
    q, scale = fr.quantize_reference(w)
    e, clamped = fr.row_exponents(w)
    amax = w.float().abs().amax(1)
    assert scale.dtype == torch.float32 and bool((torch.frexp(scale)[0] == 0.5).all())            # powers of two
    assert clamped.tolist() == [n == N - 2 for n in range(N)]                                      # only the subnormal row meets the clamp
    ratio = (amax.double() / scale.double())
    live = (amax > 0) & ~clamped
    assert bool(((ratio > 224) & (ratio <= 448))[live].all())                                      # e is the smallest with amax <= 448 * 2^e
    qmax = q.view(fr.E4M3).float().abs().amax(1)
    assert bool(((qmax >= 224) & (qmax <= 448))[live].all()) and bool(torch.isfinite(q.view(fr.E4M3).float()).all())
    print("largest |q| per row: %d of %d rows at exactly 224 (an amax / scale of 225 .. 232 rounds down)" % (int((qmax == 224).sum()), N))
    assert float(qmax[N - 1]) == 224.0 and float(ratio[N - 1]) == 225.0
    wd = fr.dequantize_reference(q, scale)                                                          # asserts that q * scale is a bf16 value
    rel = (wd.double() - w.double()).norm(dim=1) / w.double().norm(dim=1).clamp_min(1e-300)
    gauss = torch.ones(N, dtype=torch.bool)
    gauss[:3] = gauss[N - 3:] = False
    print("relative L2 error of the Gaussian rows: %.4f .. %.4f" % (float(rel[gauss].min()), float(rel[gauss].max())))
    assert float(rel[gauss].max()) < 0.04
    # the all-zero row
    assert float(scale[0]) == 1.0 and not bool(q[0].any())
    # the outlier row: the outlier is kept, the rest of the row pays for it
    assert float(wd[1].float().abs().max()) == 288.0 or float(wd[1].float().abs().max()) == 320.0
    # both sides of a boundary: amax = 448 * 2^-4 exactly keeps e = -4 and becomes 448 (0x7e); the next bf16 above takes e = -3
    assert int(e[2]) == -4 and int(q[2].max()) in (0x7e, 0xfe) and float(wd[2].float().abs().max()) == 28.0
    assert int(e[N - 3]) == -3 and float(ratio[N - 3]) == 225.0
    # the row of bf16 subnormals: e stops at -126; multiples of 2^-133 become multiples of 2^-7 and come back unchanged where e4m3 holds them
    assert int(e[N - 2]) == -126 and float(scale[N - 2]) == 2.0 ** -126
    small = w[N - 2].float().abs() <= 16 * 2.0 ** -133
    assert bool(small.any()) and wd[N - 2][small].equal(w[N - 2][small])
    # W' quantises to itself (as values: a row whose largest |q| is 224 takes the next smaller scale and twice the q)
    assert fr.dequantize_reference(*fr.quantize_reference(wd)).equal(wd)


def test_exponent_rule_is_the_smallest_power_for_every_bf16_magnitude():
    """Every positive finite bf16 as a one-element row: 448 * 2^e >= amax > 448 * 2^(e - 1) wherever e is inside the clamp"""
    bits = torch.arange(1, 0x7f80, dtype=torch.int32).to(torch.int16)
    w = bits.view(BF16)[:, None]
    e, clamped = fr.row_exponents(w)
    a = w[:, 0].double()
    hi, lo = 448.0 * torch.exp2(e.double()), 224.0 * torch.exp2(e.double())
    assert bool(((a <= hi) & (a > lo))[~clamped].all())
    assert bool((a[clamped] <= 448.0 * 2.0 ** -126).all()) and int(clamped.sum()) > 127


# ---- the GEMV mutants of this mode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", fr.GEMV_SHAPES)
def test_gemv_mutants_outside_the_bound_emulation_inside(M, N, K):
    for opt in fr.GEMV_OPTS:
        x, qs, ws, kw, res = fr.gemv_option(M, N, K, opt)
        e = [fr.row_exponents(w)[0] for w in ws]
        assert all(bool((ei != ei[fr.neighbour(len(ei))]).all()) and int(ei.max() - ei.min()) >= 6 for ei in e)      # neighbouring scales differ, spread 2^+-3
        ref, bound = lr.gemv_reference(x, ws, residual=res, **kw)
        emu, _ = lr.gemv_reference(x, ws, residual=res, emulate=True, **kw)
        worst = lr.bound_check(emu, ref, bound)[0]
        assert worst <= 1.0, (opt, worst)
        for mutant in fr.GEMV_E4M3_MUTANTS:
            bad_w = [fr.mutant_weights(q, s, mutant) for q, s in qs]
            bad, _ = lr.gemv_reference(x, bad_w, residual=res, **kw)
            w_bad = lr.bound_check(bad, ref, bound)[0]
            assert w_bad > 1.0, (opt, mutant, w_bad)
        print("gemv e4m3 %s M %d N %d K %d: emulation %.3f of the bound, mutants outside" % (opt, M, N, K, worst))


# ---- symbols, refusals ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_hold_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "walkgpt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
    from walkgpt_amd import _lib
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())


def refusal_cases(h, buf):
    """name in wg_last_error() -> calls that must return < 0 before any pointer is read (buf: a 16-byte aligned address, never dereferenced)"""
    odd = buf + 2
    gemv = lambda *a: h.wg_llama_gemv_e4m3(*a)
    lora = lambda *a: h.wg_llama_gemv_lora_e4m3(*a)
    ok = [buf, 128, buf, buf, 4, None, None, 0, None, None, 0, 128, None, 0.0, None, 0, buf, 4, 0, 0, 1]

    def edit(**kw):
        names = ["x", "ldx", "w0", "s0", "n0", "w1", "s1", "n1", "w2", "s2", "n2", "K", "gamma", "eps", "res", "ldr", "out", "ldo", "f32", "pair", "M"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    gemv_bad = [edit(x=None), edit(M=9), edit(K=192, ldx=192), edit(w1=buf, s1=buf, n1=5, pair=1), edit(ldo=3), edit(s0=None), edit(s0=odd),
                edit(w1=buf, n1=4, s1=None, ldo=8), edit(w1=buf, n1=4, s1=odd, ldo=8), edit(w0=odd)]
    tail_ok = [buf, None, None, 8, buf, 24, None]
    return {
        "llama_quantize_weight_e4m3": [lambda: h.wg_llama_quantize_weight_e4m3(None, buf, buf, 4, 128, None),
                                       lambda: h.wg_llama_quantize_weight_e4m3(buf, buf, None, 4, 128, None),
                                       lambda: h.wg_llama_quantize_weight_e4m3(buf, buf, buf, 4, 24, None),
                                       lambda: h.wg_llama_quantize_weight_e4m3(buf, buf, buf, 0, 128, None),
                                       lambda: h.wg_llama_quantize_weight_e4m3(buf, odd, buf, 4, 128, None)],
        "llama_dequantize_weight_bf16": [lambda: h.wg_llama_dequantize_weight_bf16(buf, None, buf, 4, 128, None),
                                         lambda: h.wg_llama_dequantize_weight_bf16(buf, buf, buf, 4, 40, None),
                                         lambda: h.wg_llama_dequantize_weight_bf16(buf, odd, buf, 4, 128, None)],
        "llama_gemv_e4m3": [lambda a=a: gemv(*a, None) for a in gemv_bad],
        "llama_gemv_lora_e4m3": [lambda a=a: lora(*a, *tail_ok) for a in gemv_bad] + [
            lambda: lora(*ok, buf, None, None, 12, buf, 36, None),              # rank
            lambda: lora(*ok, buf, None, None, 8, None, 24, None),              # t missing
            lambda: lora(*ok, None, buf, None, 8, buf, 24, None),               # an adapter on an absent segment
            lambda: lora(*ok, buf, None, None, 8, buf, 20, None),               # ldt
            lambda: lora(*edit(w1=buf, s1=buf, n1=4, pair=1), buf, None, None, 8, buf, 24, None)],      # pair
    }


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from walkgpt_amd import _lib
    h = _lib.lib()
    buf = (torch.zeros(1 << 14, dtype=torch.float32)).data_ptr()
    for word, calls in refusal_cases(h, buf).items():
        for i, call in enumerate(calls):
            rc = call()
            assert rc < 0 and word.encode() in h.wg_last_error(), (word, i, rc, h.wg_last_error())


# ---- host logic -----------------------------------------------------------------------------------------------------------------------
def test_weights_argument_is_validated_before_anything_else():
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    from walkgpt_amd.llama_hip import LlamaHipRunner, check_weight_mode
    assert check_weight_mode("bf16") == "bf16" and check_weight_mode("e4m3") == "e4m3"
    llm = lr.tiny_llm(96, dtype=torch.float32)                      # a CPU fp32 model: supports() would refuse it, the mode is looked at first
    for bad in ("int8", "fp8", None, "E4M3"):
        with pytest.raises(ValueError, match=r'"bf16" or "e4m3"'):
            LlamaHipRunner(llm, weights=bad)
    with pytest.raises(ValueError, match="bf16 on a GPU"):
        LlamaHipRunner(llm, weights="e4m3")
    m = walkgptForCausalLM.__new__(walkgptForCausalLM)
    nn.Module.__init__(m)
    m.llm = llm
    with pytest.raises(ValueError, match=r'"bf16" or "e4m3"'):
        m.enable_hip_llm(weights="int4")
    with pytest.raises(ValueError, match="bf16 on a GPU"):
        m.enable_hip_llm(weights="e4m3")
    assert m.hip_llm_enabled is False and m.enable_hip_llm(False, weights="e4m3") is m


def test_store_rebuilds_only_what_changed():
    from walkgpt_amd.llama_hip import WeightStore, tensor_key
    calls = []

    def quantize(t):
        calls.append(t.data_ptr())
        return t.clone(), t.sum()

    ts = [torch.full((4, 4), float(i)) for i in range(5)]
    st = WeightStore(quantize)
    assert len(st) == 0 and st.builds == 0                        # nothing is built before the first use
    st.refresh(ts)
    assert st.builds == 5 and len(st) == 5 and all(st[t][0].equal(t) for t in ts)
    kept = [st[t] for t in ts]
    st.refresh(ts)
    assert st.builds == 5 and all(st[t] is k for t, k in zip(ts, kept))              # unchanged keys: the same objects, nothing rebuilt
    ts[2].mul_(2.0)                                                # an in-place edit moves _version: that entry alone is rebuilt
    with pytest.raises(KeyError):
        st[ts[2]]
    st.refresh(ts)
    assert st.builds == 6 and calls[-1] == ts[2].data_ptr() and st[ts[2]][0].equal(ts[2]) and float(st[ts[2]][1]) == 64.0
    assert all(st[t] is k for i, (t, k) in enumerate(zip(ts, kept)) if i != 2) and len(st) == 5
    old = ts[4]
    ts[4] = torch.full((4, 4), 9.0)                                # a replaced tensor: a new entry, the old one is dropped
    st.refresh(ts)
    assert st.builds == 7 and len(st) == 5 and float(st[ts[4]][1]) == 144.0
    with pytest.raises(KeyError):
        st[old]
    st.refresh(ts + [ts[0]])                                       # a tensor named twice (tied weights) is one entry
    assert st.builds == 7 and len(st) == 5
    assert tensor_key(ts[0]) == (ts[0].data_ptr(), ts[0]._version, torch.float32)
