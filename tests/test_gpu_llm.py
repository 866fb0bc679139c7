"""The HIP LLaMA generate path on the GPU: every kernel of csrc/llama.hip against the float64 references and derived bounds of
tests/llm_reference.py, the whole tiny model against transformers' own LlamaForCausalLM in fp32 (calibrated by the same model in bf16 on
stock PyTorch), the public switch, and one layer at the 7B widths.  Every case prints its figures (pytest -s)."""
import functools
import math

import pytest
import torch

from tests import attn_reference as ar
from tests import llm_reference as lr
from walkgpt_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _report(what, worst, share):
    print("llm bound: %s  worst %.3f of the bound, %.4f of the elements beyond it" % (what, worst, share))
    assert worst <= 1.0, "%s: %.2f x the bound, %.2f %% of the elements beyond it" % (what, worst, 100 * share)


def _i32(dev, *v):
    return torch.tensor(v, device=dev, dtype=torch.int32)


# ---- rmsnorm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 4096])
def test_rmsnorm(dev, D):
    x, w = lr.rand_bf16((3, D), 1, 2.0), lr.rand_bf16((D,), 2) + 1
    ref, bound = lr.rmsnorm_reference(x, w, 1e-5)
    out = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5)
    _report("rmsnorm D %d" % D, *lr.bound_check(out, ref, bound))
    # the slot form writes row r to out[r, slot] and nothing else
    buf = torch.full((3, 4, D), 7.0, device=dev, dtype=BF16)
    ops.rmsnorm(x.to(dev), w.to(dev), 1e-5, out=buf, slot=_i32(dev, 2))
    assert buf[:, 2].equal(out) and bool((buf[:, [0, 1, 3]] == 7).all())
    ops.rmsnorm(x.to(dev), w.to(dev), 1e-5, out=buf, slot=_i32(dev, 99))            # a garbage slot is clamped into the buffer
    assert buf[:, 3].equal(out)


# ---- rope + cache ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past,L", [(0, 1), (0, 65), (70, 1), (70, 65)])
def test_rope_cache(dev, past, L):
    rows, heads, cap = 2, 2, 192
    H = heads * 128
    qkv = lr.rand_bf16((rows * L, 3 * H), 3)
    from walkgpt_amd.llama_hip import rope_table
    cos, sin = rope_table(lr.tiny_config(), cap)
    POISON = -77.0
    kc = torch.full((rows, cap, H), POISON, device=dev, dtype=BF16)
    vc = torch.full((rows, cap, H), POISON, device=dev, dtype=BF16)
    q = torch.empty(rows * L, H, device=dev, dtype=BF16)
    ops.llama_rope_cache(qkv.to(dev), cos.to(dev), sin.to(dev), _i32(dev, past), q, kc, vc, rows, L, heads)
    pos = past + torch.arange(L)
    x3 = qkv.reshape(rows, L, 3 * H)
    qref, qb = lr.rope_reference(x3[..., :H], pos)
    kref, kb = lr.rope_reference(x3[..., H:2 * H], pos)
    _report("rope q past %d L %d" % (past, L), *lr.bound_check(q, qref, qb))
    _report("rope k past %d L %d" % (past, L), *lr.bound_check(kc[:, past:past + L], kref, kb))
    assert vc[:, past:past + L].cpu().equal(x3[..., 2 * H:])
    for c in (kc, vc):                                                # slots beside the written ones keep the poison
        assert bool((c[:, :past] == POISON).all()) and bool((c[:, past + L:] == POISON).all())


# ---- attention ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attn_case(L, Lk, seed=40):
    """rows 2, heads 2: q [2, L, 256] scaled by 3 (attn_reference.mha_inputs), k / v [2, Lk, 256]; row 1's keys 5 .. 18 masked"""
    q = ar.rand_bf16((2, L, 256), seed, 3.0)
    k, v = ar.rand_bf16((2, Lk, 256), seed + 1), ar.rand_bf16((2, Lk, 256), seed + 2)
    return q, k, v, lr.attn_mask_rows(2, Lk)


def _cache(dev, k, v, mask, cap):
    rows, Lk, H = k.shape
    kc = torch.full((rows, cap, H), float("nan"), device=dev, dtype=BF16)      # unwritten slots may hold anything: NaN must not leak
    vc = torch.full((rows, cap, H), float("nan"), device=dev, dtype=BF16)
    kc[:, :Lk], vc[:, :Lk] = k.to(dev), v.to(dev)
    m = torch.ones(rows, cap, device=dev, dtype=torch.uint8)
    m[:, :Lk] = mask.to(dev, torch.uint8)
    return kc, vc, m


@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("past", [0, 40])
def test_attn_prefill(dev, L, past):
    q, k, v, mask = _attn_case(L, past + L)
    ref, A = lr.attn_reference(q, k, v, 2, mask, past)
    kc, vc, m = _cache(dev, k, v, mask, 192)
    out = ops.llama_attn_prefill(q.reshape(2 * L, 256).to(dev), kc, vc, m, _i32(dev, past), L, 2, 1 / math.sqrt(128))
    worst, share = ar.check(out.reshape(2, L, 256), ref, A)
    _report("attn_prefill L %d past %d" % (L, past), worst, share)


@pytest.mark.parametrize("past", [0, 1, 63, 64, 127, 128, 200])
def test_attn_decode(dev, past):
    q, k, v, mask = _attn_case(1, past + 1)
    ref, A = lr.attn_reference(q, k, v, 2, mask, past)
    kc, vc, m = _cache(dev, k, v, mask, 256)
    out = ops.llama_attn_decode(q.reshape(2, 256).to(dev), kc, vc, m, _i32(dev, past), 2, 1 / math.sqrt(128))
    _report("attn_decode past %d" % past, *ar.check(out.reshape(2, 1, 256), ref, A))
    if past == 200:                                                   # a garbage key count is clamped to the cache, not followed out of it
        kc2, vc2 = torch.nan_to_num(kc, nan=0.0), torch.nan_to_num(vc, nan=0.0)
        big = ops.llama_attn_decode(q.reshape(2, 256).to(dev), kc2, vc2, m, _i32(dev, 1 << 30), 2, 1 / math.sqrt(128))
        assert bool(torch.isfinite(big.float()).all())


# ---- gemv -----------------------------------------------------------------------------------------------------------------------------
def _gemv_inputs(M, N, K, nseg, seed=7):
    x = lr.rand_bf16((M, K), seed, 1.5)
    ws = [lr.rand_bf16((N + (i if N % 2 else 0), K), seed + 1 + i, 0.05) for i in range(nseg)]     # the odd N gets unequal segments
    gamma = lr.rand_bf16((K,), seed + 5, 0.3) + 1
    return x, ws, gamma


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N,K", [(256, 256), (97, 128), (512, 384)])
@pytest.mark.parametrize("opt", ["plain1", "plain2", "plain3", "norm", "residual", "pair", "f32", "norm_pair", "norm_f32"])
def test_gemv(dev, M, N, K, opt):
    nseg = {"plain1": 1, "plain2": 2, "plain3": 3, "norm": 3, "residual": 1, "f32": 1, "norm_f32": 1}.get(opt, 2)
    x, ws, gamma = _gemv_inputs(M, N, K, nseg)
    pair = "pair" in opt
    if pair:
        ws = [ws[0], ws[1][:ws[0].shape[0]].contiguous()]
    kw = dict(gamma=gamma if "norm" in opt else None, eps=1e-5, pair=pair, out_f32="f32" in opt)
    ntot = ws[0].shape[0] if pair else sum(w.shape[0] for w in ws)
    res = lr.rand_bf16((M, ntot), 19) if opt == "residual" else None
    ref, bound = lr.gemv_reference(x, ws, residual=res, **kw)
    gkw = dict(kw, gamma=None if kw["gamma"] is None else gamma.to(dev))
    if res is None:
        out = ops.llama_gemv(x.to(dev), [w.to(dev) for w in ws], **gkw)
    else:                                                             # the residual in place, as the decode step uses it
        out = res.to(dev)
        ops.llama_gemv(x.to(dev), [w.to(dev) for w in ws], residual=out, out=out, **gkw)
    _report("gemv %s M %d N %d K %d" % (opt, M, ntot, K), *lr.bound_check(out, ref, bound))


# ---- token pick -----------------------------------------------------------------------------------------------------------------------
def _pick_setup(dev, rows, V, H, cap, past, n_new):
    embed = lr.rand_bf16((V, H), 23).to(dev)
    return dict(embed=embed, x=torch.zeros(rows, H, device=dev, dtype=BF16), tokens=torch.full((rows, 16), -1, device=dev, dtype=torch.int64),
                finished=torch.zeros(rows, device=dev, dtype=torch.int32), mask=torch.zeros(rows, cap, device=dev, dtype=torch.uint8),
                state=_i32(dev, past, n_new))


def _pick(s, logits, eos, pad):
    ops.llama_pick_token(logits, s["embed"], s["x"], s["tokens"], s["finished"], s["mask"], s["state"], eos, pad)


def test_pick_token(dev):
    rows, V, H, cap = 3, 97, 256, 64
    s = _pick_setup(dev, rows, V, H, cap, 10, 0)
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(rows, V, generator=g)
    logits[0, 40] = logits[0, 77] = 9.0                               # a tie: the lowest index wins
    logits[1, 96] = 9.0                                               # the tail element
    logits[2, 5] = 9.0                                                # eos
    fin = [False] * rows
    want = lr.pick_reference(logits, fin, 5, 2)
    assert want == [40, 96, 5]
    _pick(s, logits.to(dev), 5, 2)
    assert s["tokens"][:, 0].tolist() == want and s["finished"].tolist() == [0, 0, 1] and s["state"].tolist() == [11, 1]
    assert s["x"].equal(s["embed"][want]) and s["mask"].sum(1).tolist() == [1, 1, 1] and bool(s["mask"][:, 11].all())
    logits2 = torch.randn(rows, V, generator=g)
    want2 = lr.pick_reference(logits2, fin, 5, 2)                     # row 2 is finished: it emits pad
    _pick(s, logits2.to(dev), 5, 2)
    assert want2[2] == 2 and s["tokens"][:, 1].tolist() == want2 and s["state"].tolist() == [12, 2] and bool((s["tokens"][:, 2:] == -1).all())
    # eos None: no pad substitution, nothing finishes
    s = _pick_setup(dev, rows, V, H, cap, 10, 0)
    s["finished"].fill_(1)
    _pick(s, logits.to(dev), None, None)
    assert s["tokens"][:, 0].tolist() == [40, 96, 5] and s["finished"].tolist() == [1, 1, 1]
    # the state stops at cap - 1 (and at the token buffer's end), whatever it held
    s = _pick_setup(dev, rows, V, H, cap, cap - 2, 15)
    _pick(s, logits.to(dev), None, None)
    assert s["state"].tolist() == [cap - 1, 16] and bool(s["mask"][:, cap - 1].all())
    _pick(s, logits.to(dev), None, None)
    assert s["state"].tolist() == [cap - 1, 16]
    s["state"].copy_(_i32(dev, 1 << 30, -5))
    _pick(s, logits.to(dev), None, None)
    assert s["state"].tolist() == [1 << 30, -5]


# ---- the whole model ------------------------------------------------------------------------------------------------------------------
L0, NEW = 72, 24


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class _Tiny:
    pass


@pytest.fixture(scope="module")
def tiny(dev):
    from walkgpt_amd.llama_hip import LlamaHipRunner
    t = _Tiny()
    t.llm = lr.tiny_llm(96, seed=0).to(dev)
    t.oracle = lr.tiny_llm(96, seed=0, dtype=torch.float32).to(dev)
    assert all(a.float().equal(b) for a, b in zip(t.llm.state_dict().values(), t.oracle.state_dict().values()))
    g = torch.Generator().manual_seed(1)
    t.table = t.llm.get_input_embeddings().weight
    t.emb = t.table[torch.randint(0, 96, (2, L0), generator=g).to(dev)]
    t.mask = lr.attn_mask_rows(2, L0).to(dev)
    t.runner = LlamaHipRunner(t.llm)
    with torch.no_grad():
        t.tokens, t.hidden = t.runner.generate(t.emb, t.mask, NEW, eos=None)
        # the final sequence, teacher-forced through the oracle and through the stock bf16 model
        t.seq = torch.cat([t.emb, t.table[t.tokens[:, :-1]]], 1)
        t.seq_mask = torch.cat([t.mask, t.mask.new_ones(2, NEW - 1)], 1)
        o = t.oracle(inputs_embeds=t.seq.float(), attention_mask=t.seq_mask, output_hidden_states=True)
        s = t.llm(inputs_embeds=t.seq, attention_mask=t.seq_mask, output_hidden_states=True)
    t.o_hidden, t.o_logits = o.hidden_states[-1], o.logits
    t.s_hidden, t.s_logits = s.hidden_states[-1], s.logits.float()
    return t


def test_prefill_vs_fp32_oracle(dev, tiny):
    with torch.no_grad():
        o = tiny.oracle(inputs_embeds=tiny.emb.float(), attention_mask=tiny.mask, output_hidden_states=True)
        s = tiny.llm(inputs_embeds=tiny.emb, attention_mask=tiny.mask, output_hidden_states=True)
        hid, logits = tiny.runner.prefill(tiny.emb, tiny.mask, all_logits=True)
    cal_h, cal_l = _rel(s.hidden_states[-1], o.hidden_states[-1]), float((s.logits.float() - o.logits).abs().max())
    got_h, got_l = _rel(hid, o.hidden_states[-1]), float((logits - o.logits).abs().max())
    print("prefill: hidden rel L2 %.3e (stock bf16 %.3e), max |dlogit| %.3e (stock bf16 %.3e)" % (got_h, cal_h, got_l, cal_l))
    assert hid.shape == (2, L0, 256) and hid.dtype == BF16 and logits.shape == (2, L0, 96) and logits.dtype == torch.float32
    assert got_h <= 1.5 * cal_h and got_l <= 1.5 * cal_l


def test_generate_teacher_forced_acceptance(dev, tiny):
    assert tiny.tokens.shape == (2, NEW) and tiny.tokens.dtype == torch.int64 and tiny.hidden.shape == (2, L0 + NEW - 1, 256)
    step_logits = tiny.o_logits[:, L0 - 1:]                           # [2, NEW, V]: position L0 - 1 + i predicts token i
    chosen = step_logits.gather(2, tiny.tokens[..., None])[..., 0]
    deficit = float((step_logits.amax(-1) - chosen).max())
    cal = float((tiny.s_logits - tiny.o_logits).abs().max())
    differ = float((step_logits.argmax(-1) != tiny.tokens).float().mean())
    print("generate: worst oracle deficit of a chosen token %.3e (stock bf16 max |dlogit| %.3e), %.3f of the positions differ from the oracle's "
          "argmax" % (deficit, cal, differ))
    assert deficit <= 2 * cal and differ <= 1 / 8


def test_decode_hidden_equals_prefill_of_the_final_sequence(dev, tiny):
    with torch.no_grad():
        hid, _ = tiny.runner.prefill(tiny.seq, tiny.seq_mask)
    cal = _rel(tiny.s_hidden, tiny.o_hidden)
    got = _rel(tiny.hidden, hid)
    print("decode vs prefill hidden states: rel L2 %.3e (stock bf16 against the oracle: %.3e)" % (got, cal))
    assert got <= 1.5 * cal


def test_graph_and_sync_every_change_no_bit(dev, tiny):
    r = tiny.runner
    with torch.no_grad():
        for kw in (dict(graph=False), dict(sync_every=1), dict(graph=False, sync_every=1)):
            tok, hid = r.generate(tiny.emb, tiny.mask, NEW, eos=None, **kw)
            assert tok.equal(tiny.tokens) and hid.equal(tiny.hidden), kw


def test_graph_replays_and_recaptures_on_a_weight_edit(dev, tiny):
    r = tiny.runner
    with torch.no_grad():
        r.generate(tiny.emb, tiny.mask, NEW, eos=None)
        n = r.captures
        tok, hid = r.generate(tiny.emb, tiny.mask, NEW, eos=None)
        assert r.captures == n and tok.equal(tiny.tokens) and hid.equal(tiny.hidden)
        w = tiny.llm.model.layers[1].mlp.down_proj.weight
        w.mul_(4.0)                                                   # exact in bf16, undone below
        try:
            tok2, hid2 = r.generate(tiny.emb, tiny.mask, NEW, eos=None)
            assert r.captures == n + 1 and not hid2.equal(tiny.hidden)
        finally:
            w.mul_(0.25)
        tok3, hid3 = r.generate(tiny.emb, tiny.mask, NEW, eos=None)
        assert r.captures == n + 2 and tok3.equal(tiny.tokens) and hid3.equal(tiny.hidden)


def test_generate_with_a_forced_eos(dev, tiny):
    """One lm_head row is replaced by the least-norm vector whose logit is +10 on the state from which row 0 picks its token 5 and -10 on the
    47 other states of the eos-free run (logits there are below 2): that token becomes the eos, row 0 finishes at step 5, row 1 never does."""
    from walkgpt_amd.llama_hip import LlamaHipRunner
    s = 5
    states = tiny.hidden[:, L0 - 1:].float().cpu().reshape(2 * NEW, 256)          # the state at position L0 - 1 + i picks token i
    target = torch.full((2 * NEW,), -10.0)
    target[s] = 10.0
    row = torch.linalg.lstsq(states, target[:, None]).solution[:, 0]
    used = set(tiny.tokens.flatten().tolist())
    e, pad = [t for t in range(2, 96) if t not in used][:2]
    llm = lr.tiny_llm(96, seed=0).to(dev)
    with torch.no_grad():
        llm.lm_head.weight[e] = row.to(dev, BF16)
        tok, hid = LlamaHipRunner(llm).generate(tiny.emb, tiny.mask, NEW, eos=e, pad=pad)
    assert tok.shape == (2, NEW) and hid.shape == (2, L0 + NEW - 1, 256)      # row 1 never finishes: the full length
    assert tok[0, :s].equal(tiny.tokens[0, :s]) and int(tok[0, s]) == e and bool((tok[0, s + 1:] == pad).all())
    assert tok[1].equal(tiny.tokens[1])
    # and when every row finishes, the result ends at that step, whatever sync_every is
    with torch.no_grad():
        for se in (3, 8):
            tok1, hid1 = LlamaHipRunner(llm).generate(tiny.emb[:1], tiny.mask[:1], NEW, eos=e, pad=pad, sync_every=se)
            assert tok1.shape == (1, s + 1) and int(tok1[0, s]) == e and hid1.shape == (1, L0 + s, 256)
            assert _rel(hid1, hid[:1, :L0 + s]) < 2e-2


def test_more_than_eight_rows_are_refused(dev, tiny):
    with pytest.raises(NotImplementedError):
        tiny.runner.generate(tiny.emb[:1].expand(9, -1, -1).contiguous(), tiny.mask[:1].expand(9, -1), 2)


# ---- through the public surface -------------------------------------------------------------------------------------------------------
def test_public_switch_generate_and_evaluate(dev):
    from walkgpt_amd.causal_lm import walkgptForCausalLM
    SEG, EOS = 90, 2
    torch.manual_seed(0)
    model = walkgptForCausalLM.from_pretrained(lr.tiny_config(96), torch_dtype=BF16, sam="vit_b", seg_token_idx=SEG, eos_token_id=EOS,
                                               evaluate_visual_input="sam")
    model.to(device=dev, dtype=BF16).eval()
    assert not model.hip_llm_enabled
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 90, (2, 20), generator=g)
    ids[:, 1] = -200
    toks = (torch.randn(2, 36, 256, generator=g) * 0.02).to(dev, BF16)
    kw = dict(images=toks, input_ids=ids.to(dev), attention_mask=torch.ones(2, 20, dtype=torch.bool, device=dev), max_new_tokens=6,
              return_dict_in_generate=True, output_hidden_states=True)
    images = torch.randn(1, 3, 1024, 1024, generator=g).to(dev, BF16)
    ev = lambda: model.evaluate(None, images, ids[:1].to(dev), [(1024, 1024)], [(448, 448)], [(300, 200)], max_new_tokens=4)
    stock, stock_ev = model.generate(**kw), ev()
    model.enable_hip_llm()
    assert model.hip_llm_enabled
    hip, hip_ev = model.generate(**kw), ev()
    assert torch.is_tensor(model.generate(images=toks, input_ids=ids.to(dev), max_new_tokens=2))
    model.enable_hip_llm(False)
    again = model.generate(**kw)
    assert again.sequences.equal(stock.sequences) and again.hidden_states[-1].equal(stock.hidden_states[-1])      # off = the stock path, bit for bit
    for a, b in ((hip.sequences, stock.sequences), (hip.hidden_states[-1], stock.hidden_states[-1])):
        assert a.dtype == b.dtype and a.shape[0] == b.shape[0] and a.dim() == b.dim()
    n = hip.sequences.shape[1] - 20
    assert 1 <= n <= 6 and hip.sequences[:, :20].cpu().equal(ids)
    assert hip.hidden_states[-1].shape[1] - hip.sequences.shape[1] == stock.hidden_states[-1].shape[1] - stock.sequences.shape[1]
    # [SEG] positions pick the same rows: the mask built from the sequences indexes the hidden states one to one
    m = model._seg_token_mask(hip.sequences, pad_right=False)
    assert m.shape[1] == hip.hidden_states[-1].shape[1]
    assert len(hip_ev) == len(stock_ev) == 4
    assert hip_ev[0][0].dtype == stock_ev[0][0].dtype and hip_ev[0][0].shape[0] == 1 and hip_ev[0][0][0, :20].cpu().equal(ids[0])
    assert hip_ev[1][0].shape[1:] == stock_ev[1][0].shape[1:] and hip_ev[1][0].dtype == stock_ev[1][0].dtype
    assert hip_ev[1][0].shape[0] == int(hip_ev[2][0][0]) and hip_ev[3][0].shape[0] == hip_ev[1][0].shape[0]
    # a model the kernels do not cover is refused with the reason
    bad = walkgptForCausalLM(lr.tiny_llm(96, num_key_value_heads=1).to(dev), grounding=model.model, seg_token_idx=SEG)
    with pytest.raises(ValueError, match="grouped-query"):
        bad.enable_hip_llm()


# ---- full width, one layer ------------------------------------------------------------------------------------------------------------
def test_full_width_one_layer(dev):
    """One layer of the 7B geometry: K = 11008 (86 steps of 128) and a vocabulary with a tail at their real sizes."""
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
    runner = LlamaHipRunner(llm)
    with torch.no_grad():
        s = llm(inputs_embeds=emb, attention_mask=mask, output_hidden_states=True)
        s_h, s_l = s.hidden_states[-1], s.logits.float()
        del s
        hid, logits = runner.prefill(emb, mask, all_logits=True)
        hid, logits = hid.clone(), logits.clone()
        tok, hid_g = runner.generate(emb, mask, 4, eos=None)
        llm.float()
        o = llm(inputs_embeds=emb.float(), attention_mask=mask, output_hidden_states=True)
    cal_h, cal_l = _rel(s_h, o.hidden_states[-1]), float((s_l - o.logits).abs().max())
    got_h, got_l = _rel(hid, o.hidden_states[-1]), float((logits - o.logits).abs().max())
    print("full width prefill: hidden rel L2 %.3e (stock bf16 %.3e), max |dlogit| %.3e (stock bf16 %.3e)" % (got_h, cal_h, got_l, cal_l))
    assert got_h <= 1.5 * cal_h and got_l <= 1.5 * cal_l
    assert tok.shape == (1, 4) and hid_g.shape == (1, 99, 4096) and hid_g[:, :96].equal(hid)
    assert int(tok[0, 0]) == int(logits[0, -1].argmax())
