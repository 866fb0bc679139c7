"""The e4m3 weight-only mode (W8A16) of the HIP LLaMA generate path on the GPU: the quantiser and dequantiser bit for bit against the torch
reference of tests/fp8w_reference.py, the byte-weight GEMVs against llm_reference.gemv_reference / lora_reference.gemv_lora_reference on the
DEQUANTISED weights (bounds unchanged), and the whole tiny model against transformers' own LlamaForCausalLM in fp32 with the dequantised
weights W' loaded (calibrated by the stock bf16 model with W'), the public switch, and one layer at the 7B widths.  What the quantisation
itself costs (against the fp32 model on the ORIGINAL weights) is printed, not asserted.  Every case prints its figures (pytest -s)."""
import itertools

import pytest
import torch

from tests import fp8w_reference as fr
from tests import llm_reference as lr
from tests import lora_reference as lo
from tests.test_fp8w_host import refusal_cases
from walkgpt_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _report(what, worst, share):
    print("fp8w bound: %s  worst %.3f of the bound, %.4f of the elements beyond it" % (what, worst, share))
    assert worst <= 1.0, "%s: %.2f x the bound, %.2f %% of the elements beyond it" % (what, worst, 100 * share)


def _dev(ts, dev):
    return [None if t is None else t.to(dev) for t in ts]


# ---- quantiser, dequantiser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(97, 128), (256, 384)])
def test_quantiser_and_dequantiser_bit_for_bit(dev, N, K):
    w = fr.quantiser_case(N, K)
    q_ref, s_ref = fr.quantize_reference(w)
    q, s = ops.llama_quantize_weight(w.to(dev))
    assert q.dtype == torch.uint8 and q.shape == (N, K) and s.dtype == torch.float32 and s.shape == (N,)
    bad = (q.cpu() != q_ref)
    print("quantiser N %d K %d: %d bytes and %d scales differ from the reference" % (N, K, int(bad.sum()), int((s.cpu() != s_ref).sum())))
    assert s.cpu().equal(s_ref) and not bool(bad.any())
    wd = ops.llama_dequantize_weight(q, s)
    want = q_ref.view(fr.E4M3).float() * s_ref[:, None]
    assert wd.dtype == BF16 and wd.cpu().float().equal(want) and wd.cpu().view(torch.int16).equal(want.to(BF16).view(torch.int16))
    # into a slice of a larger buffer, as the prefill uses it: nothing beside it is written
    buf = torch.full((N * K + 64,), 7.0, device=dev, dtype=BF16)
    ops.llama_dequantize_weight(q, s, out=buf[:N * K].view(N, K))
    assert buf[:N * K].view(N, K).equal(wd) and bool((buf[N * K:] == 7).all())


# ---- gemv on byte weights -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", fr.GEMV_SHAPES)
@pytest.mark.parametrize("opt", fr.GEMV_OPTS)
def test_gemv_e4m3(dev, M, N, K, opt):
    x, qs, ws, kw, res = fr.gemv_option(M, N, K, opt)
    ref, bound = lr.gemv_reference(x, ws, residual=res, **kw)
    gkw = dict(kw, gamma=None if kw["gamma"] is None else kw["gamma"].to(dev))
    qd, sd = [q.to(dev) for q, _ in qs], [s.to(dev) for _, s in qs]
    if res is None:
        out = ops.llama_gemv(x.to(dev), qd, scales=sd, **gkw)
    else:                                                             # the residual in place, as the decode step uses it
        out = res.to(dev)
        ops.llama_gemv(x.to(dev), qd, scales=sd, residual=out, out=out, **gkw)
    _report("gemv e4m3 %s M %d N %d K %d" % (opt, M, ref.shape[1], K), *lr.bound_check(out, ref, bound))


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N,K", [(97, 128), (256, 384)])
@pytest.mark.parametrize("r", [8, 16])
def test_gemv_lora_e4m3(dev, M, N, K, r):
    """The adapter rows have waves of their own, the launch's first: r = 8 with one adapter gives two adapter waves (the W rows start in
    the middle of a workgroup), with three six; with 97 + 98 + 99 = 294 W rows the last W wave holds two rows."""
    POISON = -77.0
    x, gamma, qs, ws = fr.gemv_case(M, N, K, 3)
    a_all = [lr.rand_bf16((r, K), 37 + i, 0.06) for i in range(3)]
    xd, gd = x.to(dev), gamma.to(dev)
    qd, sd, wd = [q.to(dev) for q, _ in qs], [s.to(dev) for _, s in qs], _dev(ws, dev)
    equal_t = []
    for adapted, norm in itertools.product(("q", "v", "qv", "qkv"), (False, True)):
        lora_a = [a if ch in adapted else None for a, ch in zip(a_all, "qkv")]
        ref, bound, t_ref, t_bound, cols = lo.gemv_lora_reference(x, ws, lora_a, gamma=gamma if norm else None, eps=1e-5)
        gkw = dict(gamma=gd if norm else None, eps=1e-5)
        t = torch.full((M, 3 * r), POISON, device=dev, dtype=torch.float32)
        out = ops.llama_gemv(xd, qd, scales=sd, lora_a=_dev(lora_a, dev), t_out=t, **gkw)
        what = "gemv lora e4m3 M %d N %d K %d r %d %s norm %s" % (M, ref.shape[1], K, r, adapted, norm)
        _report(what + ": out", *lr.bound_check(out, ref, bound))
        _report(what + ": t", *lr.bound_check(t[:, cols.to(dev)], t_ref[:, cols], t_bound[:, cols]))
        absent = torch.ones(3 * r, dtype=torch.bool)
        absent[cols] = False
        assert bool((t[:, absent.to(dev)] == POISON).all()), what                  # the columns of an absent adapter are left as they were
        assert out.equal(ops.llama_gemv(xd, qd, scales=sd, **gkw)), what              # the W columns: the plain byte-weight kernel's bits
        t16 = torch.full((M, 3 * r), POISON, device=dev, dtype=torch.float32)
        ops.llama_gemv(xd, wd, lora_a=_dev(lora_a, dev), t_out=t16, **gkw)
        equal_t.append(bool(t.equal(t16)))
    print("gemv lora e4m3 M %d N %d K %d r %d: t bit-equal to the bf16 entry's t in %d of %d cases" % (M, 294 if N == 97 else 3 * N, K, r,
                                                                                                    sum(equal_t), len(equal_t)))
    out = ops.llama_gemv(xd, qd, scales=sd, gamma=gd, eps=1e-5, lora_a=[None, None, None])
    assert out.equal(ops.llama_gemv(xd, qd, scales=sd, gamma=gd, eps=1e-5))


def test_entry_points_refuse_bad_arguments_and_launch_nothing(dev):
    from walkgpt_amd import _lib
    h = _lib.lib()
    buf = torch.full((1 << 14,), 3.0, device=dev, dtype=torch.float32)
    n = 0
    for word, calls in refusal_cases(h, buf.data_ptr()).items():
        for i, call in enumerate(calls):
            rc = call()
            assert rc < 0 and word.encode() in h.wg_last_error(), (word, i, rc, h.wg_last_error())
            n += 1
    torch.cuda.synchronize()
    assert bool((buf == 3.0).all())                                   # every operand pointed into this buffer: nothing was written
    print("refusals: %d calls, each < 0 with its entry's name" % n)


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
L0, NEW = 72, 24


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class _Tiny:
    pass


def _fixture(dev, llm, label):
    """llm: the bf16 model with its ORIGINAL weights (the runner quantises them itself); the oracle is its fp32 twin with W' loaded, the
    calibration the stock bf16 model with W'."""
    from walkgpt_amd.llama_hip import LlamaHipRunner
    t = _Tiny()
    t.label = label
    t.llm = llm
    t.stock = fr.dequantized_copy(llm)
    t.oracle = fr.dequantized_copy(llm).float()
    assert all(a.float().equal(b) for a, b in zip(t.stock.state_dict().values(), t.oracle.state_dict().values()))
    changed = sum(not a.equal(b) for a, b in zip(t.stock.state_dict().values(), llm.state_dict().values()))
    assert changed == 7 * len(llm.model.layers)                       # the projections, and nothing else, differ from the original
    g = torch.Generator().manual_seed(1)
    t.table = llm.get_input_embeddings().weight
    t.emb = t.table[torch.randint(0, 96, (2, L0), generator=g).to(dev)]
    t.mask = lr.attn_mask_rows(2, L0).to(dev)
    t.runner = LlamaHipRunner(llm, weights="e4m3")
    with torch.no_grad():
        t.tokens, t.hidden = t.runner.generate(t.emb, t.mask, NEW, eos=None)
        t.seq = torch.cat([t.emb, t.table[t.tokens[:, :-1]]], 1)
        t.seq_mask = torch.cat([t.mask, t.mask.new_ones(2, NEW - 1)], 1)
        o = t.oracle(inputs_embeds=t.seq.float(), attention_mask=t.seq_mask, output_hidden_states=True)
        s = t.stock(inputs_embeds=t.seq, attention_mask=t.seq_mask, output_hidden_states=True)
    t.o_hidden, t.o_logits = o.hidden_states[-1], o.logits
    t.s_hidden, t.s_logits = s.hidden_states[-1], s.logits.float()
    return t


@pytest.fixture(scope="module")
def tiny(dev):
    return _fixture(dev, lr.tiny_llm(96, seed=0).to(dev), "plain")


@pytest.fixture(scope="module")
def tiny_lora(dev):
    llm = lo.inject_lora(lr.tiny_llm(96, seed=0), ("q_proj", "v_proj"), 8, 16, 11, 0.06, {"q_proj": 0.25, "v_proj": 0.02}).to(dev)
    t = _fixture(dev, llm, "q, v adapters r 8")
    assert t.runner._rank() == 8 and len(lo.lora_layers(t.oracle)) == 4      # the oracle computes W' x + s B (A x) in fp32
    return t


def _prefill_check(t):
    with torch.no_grad():
        o = t.oracle(inputs_embeds=t.emb.float(), attention_mask=t.mask, output_hidden_states=True)
        s = t.stock(inputs_embeds=t.emb, attention_mask=t.mask, output_hidden_states=True)
        hid, logits = t.runner.prefill(t.emb, t.mask, all_logits=True)
    cal_h, cal_l = _rel(s.hidden_states[-1], o.hidden_states[-1]), float((s.logits.float() - o.logits).abs().max())
    got_h, got_l = _rel(hid, o.hidden_states[-1]), float((logits - o.logits).abs().max())
    print("e4m3 prefill (%s): hidden rel L2 %.3e (stock bf16 on W' %.3e), max |dlogit| %.3e (stock bf16 on W' %.3e)"
          % (t.label, got_h, cal_h, got_l, cal_l))
    assert hid.shape == (2, L0, 256) and hid.dtype == BF16 and logits.shape == (2, L0, 96) and logits.dtype == torch.float32
    assert got_h <= 1.5 * cal_h and got_l <= 1.5 * cal_l


def _teacher_forced_check(t):
    assert t.tokens.shape == (2, NEW) and t.tokens.dtype == torch.int64 and t.hidden.shape == (2, L0 + NEW - 1, 256)
    step_logits = t.o_logits[:, L0 - 1:]                              # [2, NEW, V]: position L0 - 1 + i predicts token i
    chosen = step_logits.gather(2, t.tokens[..., None])[..., 0]
    deficit = float((step_logits.amax(-1) - chosen).max())
    cal = float((t.s_logits - t.o_logits).abs().max())
    differ = float((step_logits.argmax(-1) != t.tokens).float().mean())
    print("e4m3 generate (%s): worst oracle deficit of a chosen token %.3e (stock bf16 on W' max |dlogit| %.3e), %.3f of the positions differ "
          "from the oracle's argmax" % (t.label, deficit, cal, differ))
    assert deficit <= 2 * cal and differ <= 1 / 8


def test_prefill_vs_fp32_oracle_on_dequantised_weights(dev, tiny):
    _prefill_check(tiny)


def test_generate_teacher_forced_acceptance(dev, tiny):
    _teacher_forced_check(tiny)


def test_decode_hidden_equals_prefill_of_the_final_sequence(dev, tiny):
    with torch.no_grad():
        hid, _ = tiny.runner.prefill(tiny.seq, tiny.seq_mask)
    cal = _rel(tiny.s_hidden, tiny.o_hidden)
    got = _rel(tiny.hidden, hid)
    print("e4m3 decode vs prefill hidden states: rel L2 %.3e (stock bf16 on W' against the oracle: %.3e)" % (got, cal))
    assert got <= 1.5 * cal


def test_graph_and_sync_every_change_no_bit(dev, tiny):
    r = tiny.runner
    with torch.no_grad():
        for kw in (dict(graph=False), dict(sync_every=1), dict(graph=False, sync_every=1)):
            tok, hid = r.generate(tiny.emb, tiny.mask, NEW, eos=None, **kw)
            assert tok.equal(tiny.tokens) and hid.equal(tiny.hidden), kw


def test_graph_replays_and_a_weight_edit_requantises_and_recaptures(dev, tiny):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    r = tiny.runner
    with torch.no_grad():
        r.generate(tiny.emb, tiny.mask, NEW, eos=None)
        n, built = r.captures, r._store.builds
        assert built >= 14 and len(r._store) == 14
        tok, hid = r.generate(tiny.emb, tiny.mask, NEW, eos=None)
        assert r.captures == n and r._store.builds == built and tok.equal(tiny.tokens) and hid.equal(tiny.hidden)
        w = tiny.llm.model.layers[1].mlp.down_proj.weight
        saved = w.clone()
        w[::2].mul_(-1.5)                                             # not a power of two: the bytes change, not only the scales
        try:
            tok2, hid2 = r.generate(tiny.emb, tiny.mask, NEW, eos=None)
            assert r.captures == n + 1 and r._store.builds == built + 1 and len(r._store) == 14 and not hid2.equal(tiny.hidden)
            tok_f, hid_f = LlamaHipRunner(tiny.llm, weights="e4m3").generate(tiny.emb, tiny.mask, NEW, eos=None)      # a fresh runner on the edited model
            assert tok2.equal(tok_f) and hid2.equal(hid_f)
        finally:
            w.copy_(saved)
        tok3, hid3 = r.generate(tiny.emb, tiny.mask, NEW, eos=None)
        assert r.captures == n + 2 and r._store.builds == built + 2 and tok3.equal(tiny.tokens) and hid3.equal(tiny.hidden)


def test_what_the_quantisation_costs_is_reported(dev, tiny):
    """Against the fp32 model on the ORIGINAL weights, teacher-forced on the e4m3 run's sequence.  Printed for profiles/llm_generate.md; a
    random-init model has near-ties everywhere, so the argmax figure overstates what a trained model would see."""
    orig = lr.tiny_llm(96, seed=0, dtype=torch.float32).to(dev)
    with torch.no_grad():
        o = orig(inputs_embeds=tiny.seq.float(), attention_mask=tiny.seq_mask)
        _, logits = tiny.runner.prefill(tiny.seq, tiny.seq_mask, all_logits=True)
    d = float((logits - o.logits).abs().max())
    d_oracle = float((tiny.o_logits - o.logits).abs().max())
    flips = float((logits.argmax(-1) != o.logits.argmax(-1)).float().mean())
    flips_oracle = float((tiny.o_logits.argmax(-1) != o.logits.argmax(-1)).float().mean())
    print("quantisation cost, tiny model: max |dlogit| %.3e on a logit std of %.3f (fp32 on W' alone: %.3e); %.3f of the argmaxes change "
          "(fp32 on W' alone: %.3f)" % (d, float(o.logits.std()), d_oracle, flips, flips_oracle))
    assert torch.isfinite(logits).all()


def test_lora_prefill_vs_fp32_oracle(dev, tiny_lora):
    _prefill_check(tiny_lora)


def test_lora_generate_teacher_forced_acceptance(dev, tiny_lora, tiny):
    _teacher_forced_check(tiny_lora)
    assert not tiny_lora.hidden.equal(tiny.hidden)                    # (the adapters are not inert)
    with torch.no_grad():
        tok, hid = tiny_lora.runner.generate(tiny_lora.emb, tiny_lora.mask, NEW, eos=None, graph=False)
    assert tok.equal(tiny_lora.tokens) and hid.equal(tiny_lora.hidden)


# ---- through the public surface -------------------------------------------------------------------------------------------------------
def test_public_switch_e4m3_and_back_to_bf16(dev):
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    SEG, EOS = 90, 2
    torch.manual_seed(0)
    model = walkgptForCausalLM.from_pretrained(lr.tiny_config(96), torch_dtype=BF16, sam="vit_b", seg_token_idx=SEG, eos_token_id=EOS,
                                               evaluate_visual_input="sam")
    model.to(device=dev, dtype=BF16).eval()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 90, (2, 20), generator=g)
    ids[:, 1] = -200
    toks = (torch.randn(2, 36, 256, generator=g) * 0.02).to(dev, BF16)
    kw = dict(images=toks, input_ids=ids.to(dev), attention_mask=torch.ones(2, 20, dtype=torch.bool, device=dev), max_new_tokens=6,
              return_dict_in_generate=True, output_hidden_states=True)
    images = torch.randn(1, 3, 1024, 1024, generator=g).to(dev, BF16)
    ev = lambda: model.evaluate(None, images, ids[:1].to(dev), [(1024, 1024)], [(448, 448)], [(300, 200)], max_new_tokens=4)
    before = {k: v.clone() for k, v in model.llm.state_dict().items()}
    model.enable_hip_llm()
    assert model._hip_llm.weights == "bf16" and model._hip_llm._store is None
    bf = model.generate(**kw)
    assert model.enable_hip_llm(weights="e4m3") is model and model.hip_llm_enabled and model._hip_llm.weights == "e4m3"
    q8, q8_ev = model.generate(**kw), ev()
    assert len(model._hip_llm._store) == 7 * len(model.llm.model.layers)
    assert q8.sequences.dtype == bf.sequences.dtype and q8.sequences[:, :20].cpu().equal(ids) and 1 <= q8.sequences.shape[1] - 20 <= 6
    assert q8.hidden_states[-1].dtype == BF16 and q8.hidden_states[-1].shape[1] - q8.sequences.shape[1] == bf.hidden_states[-1].shape[1] - bf.sequences.shape[1]
    assert len(q8_ev) == 4 and q8_ev[0][0][0, :20].cpu().equal(ids[0]) and q8_ev[1][0].shape[0] == int(q8_ev[2][0][0])
    assert torch.is_tensor(model.generate(images=toks, input_ids=ids.to(dev), max_new_tokens=2))
    model.enable_hip_llm(weights="bf16")                              # back: the bf16 tokens bit for bit, no store
    assert model._hip_llm.weights == "bf16" and model._hip_llm._store is None
    again = model.generate(**kw)
    assert again.sequences.equal(bf.sequences) and again.hidden_states[-1].equal(bf.hidden_states[-1])
    model.enable_hip_llm(weights="e4m3")
    model.enable_hip_llm(False)
    assert model._hip_llm is None and not model.hip_llm_enabled
    with pytest.raises(ValueError, match='"bf16" or "e4m3"'):
        model.enable_hip_llm(weights="int8")
    assert all(v.equal(before[k]) for k, v in model.llm.state_dict().items())          # the model's own tensors were never touched


# ---- full width, one layer ------------------------------------------------------------------------------------------------------------
def test_full_width_one_layer_e4m3(dev):
    """One layer of the 7B geometry: K = 4096 (4 sweeps of 1024) and K = 11008 (10 sweeps and one of 48 lanes), against the model with the
    dequantised weights.  The weights are dequantised by the kernels here (pinned bit for bit by the quantiser test above)."""
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
    g = torch.Generator().manual_seed(2)
    emb = llm.get_input_embeddings().weight[torch.randint(0, 32007, (1, 96), generator=g).to(dev)]
    mask = torch.ones(1, 96, dtype=torch.bool, device=dev)
    runner = LlamaHipRunner(llm, weights="e4m3")
    with torch.no_grad():
        hid, logits = runner.prefill(emb, mask, all_logits=True)
        hid, logits = hid.clone(), logits.clone()
        tok, hid_g = runner.generate(emb, mask, 4, eos=None)
        o0 = llm(inputs_embeds=emb, attention_mask=mask).logits.float()          # the stock bf16 model on the original weights
        layer = llm.model.layers[0]
        for m in (layer.self_attn.q_proj, layer.self_attn.k_proj, layer.self_attn.v_proj, layer.self_attn.o_proj, layer.mlp.gate_proj,
                  layer.mlp.up_proj, layer.mlp.down_proj):
            m.weight.copy_(ops.llama_dequantize_weight(*ops.llama_quantize_weight(m.weight)))
        s = llm(inputs_embeds=emb, attention_mask=mask, output_hidden_states=True)
        s_h, s_l = s.hidden_states[-1], s.logits.float()
        del s
        llm.float()
        o = llm(inputs_embeds=emb.float(), attention_mask=mask, output_hidden_states=True)
    cal_h, cal_l = _rel(s_h, o.hidden_states[-1]), float((s_l - o.logits).abs().max())
    got_h, got_l = _rel(hid, o.hidden_states[-1]), float((logits - o.logits).abs().max())
    print("e4m3 full width prefill: hidden rel L2 %.3e (stock bf16 on W' %.3e), max |dlogit| %.3e (stock bf16 on W' %.3e); the quantisation "
          "moves the stock bf16 logits by up to %.3e" % (got_h, cal_h, got_l, cal_l, float((s_l - o0).abs().max())))
    assert got_h <= 1.5 * cal_h and got_l <= 1.5 * cal_l
    assert tok.shape == (1, 4) and hid_g.shape == (1, 99, 4096) and hid_g[:, :96].equal(hid)
    assert int(tok[0, 0]) == int(logits[0, -1].argmax())
