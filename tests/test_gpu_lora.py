"""Unmerged LoRA adapters on the HIP LLaMA generate path, on the GPU: the two extended kernels against the float64 references and derived
bounds of tests/lora_reference.py, the whole tiny model with adapters against transformers' own LlamaForCausalLM in fp32 with the same
adapters (calibrated by the same adapted model in bf16 on stock PyTorch), the public switch on a PEFT-shaped wrapper, and one layer at the
7B widths.  Every case prints its figures (pytest -s)."""
import itertools

import pytest
import torch
from torch import nn

from tests import llm_reference as lr
from tests import lora_reference as lo
from walkgpt_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SUBSETS = ("q", "v", "qv", "qkv")


def _report(what, worst, share):
    print("lora bound: %s  worst %.3f of the bound, %.4f of the elements beyond it" % (what, worst, share))
    assert worst <= 1.0, "%s: %.2f x the bound, %.2f %% of the elements beyond it" % (what, worst, 100 * share)


def _i32(dev, *v):
    return torch.tensor(v, device=dev, dtype=torch.int32)


def _dev(ts, dev):
    return [None if t is None else t.to(dev) for t in ts]


# ---- gemv with adapter rows -----------------------------------------------------------------------------------------------------------
def _gemv_inputs(M, N, K, r, seed=7):
    """x, three weights and gamma as test_gpu_llm._gemv_inputs makes them (the odd N gets unequal segments: 97 + 98 + 99 = 294 columns, no
    multiple of 4, so one wave holds the last two W rows and the first two A rows), and an A [r, K] per segment"""
    x = lr.rand_bf16((M, K), seed, 1.5)
    ws = [lr.rand_bf16((N + (i if N % 2 else 0), K), seed + 1 + i, 0.05) for i in range(3)]
    gamma = lr.rand_bf16((K,), seed + 5, 0.3) + 1
    return x, ws, gamma, [lr.rand_bf16((r, K), seed + 30 + i, 0.06) for i in range(3)]


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N,K", [(97, 128), (256, 384)])
@pytest.mark.parametrize("r", [8, 16])
def test_gemv_lora(dev, M, N, K, r):
    POISON = -77.0
    x, ws, gamma, a_all = _gemv_inputs(M, N, K, r)
    assert (sum(w.shape[0] for w in ws) % 4 != 0) == (N == 97)
    xd, wd, gd = x.to(dev), _dev(ws, dev), gamma.to(dev)
    for adapted, norm in itertools.product(SUBSETS, (False, True)):
        lora_a = [a if ch in adapted else None for a, ch in zip(a_all, "qkv")]
        kw = dict(gamma=gamma if norm else None, eps=1e-5)
        ref, bound, t_ref, t_bound, cols = lo.gemv_lora_reference(x, ws, lora_a, **kw)
        gkw = dict(gamma=gd if norm else None, eps=1e-5)
        t = torch.full((M, 3 * r), POISON, device=dev, dtype=torch.float32)
        out = ops.llama_gemv(xd, wd, lora_a=_dev(lora_a, dev), t_out=t, **gkw)
        what = "gemv lora M %d N %d K %d r %d %s norm %s" % (M, ref.shape[1], K, r, adapted, norm)
        _report(what + ": out", *lr.bound_check(out, ref, bound))
        _report(what + ": t", *lr.bound_check(t[:, cols.to(dev)], t_ref[:, cols], t_bound[:, cols]))
        absent = torch.ones(3 * r, dtype=torch.bool)
        absent[cols] = False
        assert bool((t[:, absent.to(dev)] == POISON).all()), what                  # the columns of an absent adapter are left as they were
        assert out.equal(ops.llama_gemv(xd, wd, **gkw)), what                        # the W columns: the plain kernel's bits


def test_gemv_lora_without_adapters_is_the_plain_gemv(dev):
    x, ws, gamma, _ = _gemv_inputs(3, 97, 128, 8)
    xd, wd, gd = x.to(dev), _dev(ws, dev), gamma.to(dev)
    out = ops.llama_gemv(xd, wd, gamma=gd, eps=1e-5, lora_a=[None, None, None])
    assert out.equal(ops.llama_gemv(xd, wd, gamma=gd, eps=1e-5))


# ---- rope + cache with the up-projection ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past,L", [(0, 1), (0, 65), (70, 1), (70, 65)])
@pytest.mark.parametrize("r", [8, 16])
def test_rope_cache_lora(dev, past, L, r):
    from walkgpt_amd.llama_hip import rope_table
    rows, heads, cap = 2, 2, 192
    H = heads * 128
    POISON = -77.0
    cos, sin = rope_table(lr.tiny_config(), cap)
    cos, sin = cos.to(dev), sin.to(dev)
    pos = past + torch.arange(L)

    def run(qkv, t, lora_b, scales):
        kc = torch.full((rows, cap, H), POISON, device=dev, dtype=BF16)
        vc = torch.full((rows, cap, H), POISON, device=dev, dtype=BF16)
        q = torch.empty(rows * L, H, device=dev, dtype=BF16)
        kw = {} if lora_b is None else dict(t=t.reshape(rows * L, -1).to(dev), lora_b=_dev(lora_b, dev), lora_scale=scales)
        ops.llama_rope_cache(qkv.reshape(rows * L, 3 * H).to(dev), cos, sin, _i32(dev, past), q, kc, vc, rows, L, heads, **kw)
        return q, kc, vc

    for adapted in SUBSETS:
        qkv, t, lora_b, scales = lo.rope_lora_inputs(rows, L, heads, r, adapted)
        (qref, qb), (kref, kb), (vref, vb) = lo.rope_lora_reference(qkv, pos, t, lora_b, scales, heads)
        q, kc, vc = run(qkv, t, lora_b, scales)
        what = "rope lora past %d L %d r %d %s" % (past, L, r, adapted)
        _report(what + ": q", *lr.bound_check(q, qref, qb))
        _report(what + ": k", *lr.bound_check(kc[:, past:past + L], kref, kb))
        if "v" in adapted:
            _report(what + ": v", *lr.bound_check(vc[:, past:past + L], vref, vb))
        else:
            assert vb is None and vc[:, past:past + L].cpu().equal(qkv[..., 2 * H:])          # an unadapted v is a copy
        for c in (kc, vc):                                            # slots beside the written ones keep the poison
            assert bool((c[:, :past] == POISON).all()) and bool((c[:, past + L:] == POISON).all())
    # all three B null: the old entry point's bits
    got, want = run(qkv, t, [None, None, None], scales), run(qkv, t, None, None)
    assert all(a.equal(b) for a, b in zip(got, want))


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
L0, NEW = 72, 24
CONFIGS = {"qv_r8": (("q_proj", "v_proj"), 8, 16), "qkv_r16": (("q_proj", "k_proj", "v_proj"), 16, 16)}
STD_A, STD_B = 0.06, {"q_proj": 0.25, "k_proj": 0.25, "v_proj": 0.02}
SEED = 11


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _adapted(dev, cfg, dtype=BF16):
    targets, r, alpha = CONFIGS[cfg]
    return lo.inject_lora(lr.tiny_llm(96, seed=0, dtype=dtype), targets, r, alpha, SEED, STD_A, STD_B).to(dev)


def _keep(llm, keep):
    """disable every adapter whose projection is not named in `keep`"""
    for name, m in llm.named_modules():
        if isinstance(m, lo.LoraLinear):
            m.disable_adapters = name.rsplit(".", 1)[-1] not in keep


class _Tiny:
    pass


@pytest.fixture(scope="module", params=list(CONFIGS))
def tiny(request, dev):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    t = _Tiny()
    t.cfg = request.param
    targets = CONFIGS[t.cfg][0]
    t.llm, t.oracle = _adapted(dev, t.cfg), _adapted(dev, t.cfg, torch.float32)
    assert all(a.float().equal(b) for a, b in zip(t.llm.state_dict().values(), t.oracle.state_dict().values()))
    assert len(lo.lora_layers(t.llm)) == 2 * len(targets)
    g = torch.Generator().manual_seed(1)
    t.table = t.llm.get_input_embeddings().weight
    t.emb = t.table[torch.randint(0, 96, (2, L0), generator=g).to(dev)]
    t.mask = lr.attn_mask_rows(2, L0).to(dev)
    t.runner = LlamaHipRunner(t.llm)
    with torch.no_grad():
        t.tokens, t.hidden = t.runner.generate(t.emb, t.mask, NEW, eos=None)
        t.seq = torch.cat([t.emb, t.table[t.tokens[:, :-1]]], 1)
        t.seq_mask = torch.cat([t.mask, t.mask.new_ones(2, NEW - 1)], 1)
        run = lambda m, x: m(inputs_embeds=x, attention_mask=t.seq_mask, output_hidden_states=True)
        o, s = run(t.oracle, t.seq.float()), run(t.llm, t.seq)
        t.o_hidden, t.o_logits = o.hidden_states[-1], o.logits
        t.s_hidden, t.s_logits = s.hidden_states[-1], s.logits.float()
        t.cal = _rel(t.s_hidden, t.o_hidden)
        # the inputs must keep every adapter visible to a model-level bound: each one alone moves the oracle's final hidden states by at
        # least 10 x the distance of the stock bf16 model from the oracle
        _keep(t.oracle, ())
        plain = run(t.oracle, t.seq.float()).hidden_states[-1]
        for name in targets:
            _keep(t.oracle, (name,))
            worth = _rel(run(t.oracle, t.seq.float()).hidden_states[-1], plain)
            print("lora fixture %s: %s alone moves the oracle's hidden states by %.3e = %.1f x the calibration %.3e" % (t.cfg, name, worth, worth / t.cal, t.cal))
            assert worth >= 10 * t.cal, (name, worth, t.cal)
        _keep(t.oracle, targets)
    return t


def test_prefill_vs_fp32_oracle(dev, tiny):
    with torch.no_grad():
        o = tiny.oracle(inputs_embeds=tiny.emb.float(), attention_mask=tiny.mask, output_hidden_states=True)
        s = tiny.llm(inputs_embeds=tiny.emb, attention_mask=tiny.mask, output_hidden_states=True)
        hid, logits = tiny.runner.prefill(tiny.emb, tiny.mask, all_logits=True)
    cal_h, cal_l = _rel(s.hidden_states[-1], o.hidden_states[-1]), float((s.logits.float() - o.logits).abs().max())
    got_h, got_l = _rel(hid, o.hidden_states[-1]), float((logits - o.logits).abs().max())
    print("lora prefill %s: hidden rel L2 %.3e (stock bf16 %.3e), max |dlogit| %.3e (stock bf16 %.3e)" % (tiny.cfg, got_h, cal_h, got_l, cal_l))
    assert hid.shape == (2, L0, 256) and hid.dtype == BF16 and logits.shape == (2, L0, 96) and logits.dtype == torch.float32
    assert got_h <= 1.5 * cal_h and got_l <= 1.5 * cal_l


def test_generate_teacher_forced_acceptance(dev, tiny):
    assert tiny.tokens.shape == (2, NEW) and tiny.tokens.dtype == torch.int64 and tiny.hidden.shape == (2, L0 + NEW - 1, 256)
    step_logits = tiny.o_logits[:, L0 - 1:]                           # [2, NEW, V]: position L0 - 1 + i predicts token i
    chosen = step_logits.gather(2, tiny.tokens[..., None])[..., 0]
    deficit = float((step_logits.amax(-1) - chosen).max())
    cal = float((tiny.s_logits - tiny.o_logits).abs().max())
    differ = float((step_logits.argmax(-1) != tiny.tokens).float().mean())
    print("lora generate %s: worst oracle deficit of a chosen token %.3e (stock bf16 max |dlogit| %.3e), %.3f of the positions differ from the "
          "oracle's argmax" % (tiny.cfg, deficit, cal, differ))
    assert deficit <= 2 * cal and differ <= 1 / 8


def test_decode_hidden_equals_prefill_of_the_final_sequence(dev, tiny):
    with torch.no_grad():
        hid, _ = tiny.runner.prefill(tiny.seq, tiny.seq_mask)
    got = _rel(tiny.hidden, hid)
    print("lora decode vs prefill hidden states %s: rel L2 %.3e (stock bf16 against the oracle: %.3e)" % (tiny.cfg, got, tiny.cal))
    assert got <= 1.5 * tiny.cal


def test_graph_and_sync_every_change_no_bit(dev, tiny):
    r = tiny.runner
    with torch.no_grad():
        for kw in (dict(graph=False), dict(sync_every=1), dict(graph=False, sync_every=1)):
            tok, hid = r.generate(tiny.emb, tiny.mask, NEW, eos=None, **kw)
            assert tok.equal(tiny.tokens) and hid.equal(tiny.hidden), kw


def test_graph_replays_and_recaptures_on_an_adapter_change(dev, tiny):
    r = tiny.runner
    gen = lambda: r.generate(tiny.emb, tiny.mask, NEW, eos=None)
    same = lambda tok, hid: tok.equal(tiny.tokens) and hid.equal(tiny.hidden)
    layers = tiny.llm.model.layers
    with torch.no_grad():
        gen()
        n = r.captures
        assert same(*gen()) and r.captures == n                      # a second generate replays
        B = layers[1].self_attn.v_proj.lora_B["default"].weight
        B.mul_(4.0)                                                   # exact in bf16, undone below
        try:
            _, hid = gen()
            assert r.captures == n + 1 and not hid.equal(tiny.hidden)
        finally:
            B.mul_(0.25)
        assert same(*gen()) and r.captures == n + 2
        q = layers[0].self_attn.q_proj
        old = q.scaling["default"]
        q.scaling["default"] = old * 2
        try:
            _, hid = gen()
            assert r.captures == n + 3 and not hid.equal(tiny.hidden)
        finally:
            q.scaling["default"] = old
        assert same(*gen()) and r.captures == n + 4
        q.disable_adapters = True
        try:
            _, hid = gen()
            assert r.captures == n + 5 and not hid.equal(tiny.hidden)
        finally:
            q.disable_adapters = False
        assert same(*gen()) and r.captures == n + 6


@pytest.mark.parametrize("how", ["B = 0", "disable_adapters"])
def test_inert_adapters_give_the_plain_model_bit_for_bit(dev, tiny, how):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    llm = _adapted(dev, tiny.cfg)
    for m in lo.lora_layers(llm):
        if how == "B = 0":
            with torch.no_grad():
                m.lora_B["default"].weight.zero_()
        else:
            m.disable_adapters = True
    runner = LlamaHipRunner(llm)
    assert (runner._rank() > 0) == (how == "B = 0")                  # zero B still runs the LoRA kernels; disabled layers take the plain ones
    with torch.no_grad():
        tok, hid = runner.generate(tiny.emb, tiny.mask, NEW, eos=None)
        tok0, hid0 = LlamaHipRunner(lr.tiny_llm(96, seed=0).to(dev)).generate(tiny.emb, tiny.mask, NEW, eos=None)
    assert tok.equal(tok0) and hid.equal(hid0)
    assert not hid0.equal(tiny.hidden)                                # (and the adapters of the fixture are not inert)


# ---- through the public surface -------------------------------------------------------------------------------------------------------
class _Forwarding(nn.Module):
    """PEFT's two shells (PeftModel.base_model = LoraModel, LoraModel.model = the model): attributes they lack come from the inner module"""

    def __init__(self, name, inner):
        super().__init__()
        self._inner_name = name
        self.add_module(name, inner)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name == "_inner_name":
                raise
            return getattr(super().__getattr__(self._inner_name), name)


def test_public_switch_on_a_peft_shaped_model(dev):
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    SEG, EOS = 90, 2
    torch.manual_seed(0)
    model = walkgptForCausalLM.from_pretrained(lr.tiny_config(96), torch_dtype=BF16, sam="vit_b", seg_token_idx=SEG, eos_token_id=EOS,
                                               evaluate_visual_input="sam")
    model.to(device=dev, dtype=BF16).eval()
    lo.inject_lora(model.llm, ("q_proj", "v_proj"), 8, 16, SEED, STD_A, STD_B)
    wrapped = _Forwarding("base_model", _Forwarding("model", model))
    assert wrapped.base_model.model is model and not wrapped.hip_llm_enabled
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 90, (2, 20), generator=g)
    ids[:, 1] = -200
    toks = (torch.randn(2, 36, 256, generator=g) * 0.02).to(dev, BF16)
    kw = dict(images=toks, input_ids=ids.to(dev), attention_mask=torch.ones(2, 20, dtype=torch.bool, device=dev), max_new_tokens=6,
              return_dict_in_generate=True, output_hidden_states=True)
    images = torch.randn(1, 3, 1024, 1024, generator=g).to(dev, BF16)
    ev = lambda: wrapped.base_model.evaluate(None, images, ids[:1].to(dev), [(1024, 1024)], [(448, 448)], [(300, 200)], max_new_tokens=4)
    stock, stock_ev = wrapped.generate(**kw), ev()
    assert wrapped.enable_hip_llm() is model
    assert wrapped.hip_llm_enabled and model._hip_llm._rank() == 8
    hip, hip_ev = wrapped.generate(**kw), ev()
    wrapped.enable_hip_llm(False)
    again = wrapped.generate(**kw)
    assert again.sequences.equal(stock.sequences) and again.hidden_states[-1].equal(stock.hidden_states[-1])      # off = the stock path, bit for bit
    for a, b in ((hip.sequences, stock.sequences), (hip.hidden_states[-1], stock.hidden_states[-1])):
        assert a.dtype == b.dtype and a.shape[0] == b.shape[0] and a.dim() == b.dim()
    n = hip.sequences.shape[1] - 20
    assert 1 <= n <= 6 and hip.sequences[:, :20].cpu().equal(ids)
    assert hip.hidden_states[-1].shape[1] - hip.sequences.shape[1] == stock.hidden_states[-1].shape[1] - stock.sequences.shape[1]
    m = model._seg_token_mask(hip.sequences, pad_right=False)         # [SEG] rows index the hidden states one to one
    assert m.shape[1] == hip.hidden_states[-1].shape[1]
    assert len(hip_ev) == len(stock_ev) == 4
    assert hip_ev[0][0].dtype == stock_ev[0][0].dtype and hip_ev[0][0].shape[0] == 1 and hip_ev[0][0][0, :20].cpu().equal(ids[0])
    assert hip_ev[1][0].shape[1:] == stock_ev[1][0].shape[1:] and hip_ev[1][0].dtype == stock_ev[1][0].dtype
    assert hip_ev[1][0].shape[0] == int(hip_ev[2][0][0]) and hip_ev[3][0].shape[0] == hip_ev[1][0].shape[0]
    # an adapter the kernels do not cover is refused with the module's name
    lo.inject_lora(model.llm, ("o_proj",), 8, 16, SEED, STD_A, 0.02)
    with pytest.raises(ValueError, match="o_proj"):
        wrapped.enable_hip_llm()
    assert not wrapped.hip_llm_enabled


# ---- full width, one layer ------------------------------------------------------------------------------------------------------------
def test_full_width_one_layer_with_adapters(dev):
    """One layer of the 7B geometry with q, v adapters at r 8: 3 * 4096 W rows and 16 A rows of K = 4096 in the q | k | v launch."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from walkgpt_amd.llama_hip import LlamaHipRunner
    cfg = LlamaConfig(vocab_size=32007, hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                      num_key_value_heads=32, rms_norm_eps=1e-5, max_position_embeddings=2048)
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        llm = LlamaForCausalLM(cfg).eval().to(dev)
    finally:
        torch.set_default_dtype(prev)
    lo.inject_lora(llm, ("q_proj", "v_proj"), 8, 16, SEED, STD_A, 0.02)
    g = torch.Generator().manual_seed(2)
    emb = llm.get_input_embeddings().weight[torch.randint(0, 32007, (1, 96), generator=g).to(dev)]
    mask = torch.ones(1, 96, dtype=torch.bool, device=dev)
    runner = LlamaHipRunner(llm)
    assert runner._rank() == 8
    with torch.no_grad():
        s = llm(inputs_embeds=emb, attention_mask=mask, output_hidden_states=True)
        s_h, s_l = s.hidden_states[-1], s.logits.float()
        del s
        hid, logits = runner.prefill(emb, mask, all_logits=True)
        hid, logits = hid.clone(), logits.clone()
        tok, hid_g = runner.generate(emb, mask, 4, eos=None)
        llm.float()
        o = llm(inputs_embeds=emb.float(), attention_mask=mask, output_hidden_states=True)
        _keep(llm, ())
        plain = llm(inputs_embeds=emb.float(), attention_mask=mask, output_hidden_states=True).hidden_states[-1]
    cal_h, cal_l = _rel(s_h, o.hidden_states[-1]), float((s_l - o.logits).abs().max())
    got_h, got_l = _rel(hid, o.hidden_states[-1]), float((logits - o.logits).abs().max())
    worth = _rel(o.hidden_states[-1], plain)
    print("lora full width prefill: hidden rel L2 %.3e (stock bf16 %.3e), max |dlogit| %.3e (stock bf16 %.3e); the adapters move the oracle by "
          "%.3e" % (got_h, cal_h, got_l, cal_l, worth))
    assert worth >= 10 * cal_h
    assert got_h <= 1.5 * cal_h and got_l <= 1.5 * cal_l
    assert tok.shape == (1, 4) and hid_g.shape == (1, 99, 4096) and hid_g[:, :96].equal(hid)
    assert int(tok[0, 0]) == int(logits[0, -1].argmax())


# ---- supports on an otherwise qualifying model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["fp32 B", "non-contiguous A"])
def test_supports_refuses_adapter_weights_that_are_not_contiguous_bf16(dev, what):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    llm = _adapted(dev, "qv_r8")
    assert LlamaHipRunner.supports(llm) == (True, "")
    m = llm.model.layers[1].self_attn.v_proj
    if what == "fp32 B":
        m.lora_B["default"].float()
    else:
        w = m.lora_A["default"].weight
        m.lora_A["default"].weight = nn.Parameter(torch.cat([w, w], 1)[:, :w.shape[1]], requires_grad=False)
        assert not m.lora_A["default"].weight.is_contiguous()
    ok, why = LlamaHipRunner.supports(llm)
    print("supports, %s: %s" % (what, why))
    assert ok is False and "layers.1.self_attn.v_proj" in why and "adapter weights must be contiguous bf16 on a GPU" in why
    with pytest.raises(ValueError, match="layers.1.self_attn.v_proj"):
        LlamaHipRunner(llm)
