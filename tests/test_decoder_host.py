"""The references of tests/decoder_reference.py checked on the CPU (no GPU, no library): every emulation inside its tolerance, every mutant
outside it by the stated margin, the merge of exact partials, and the float64 chain of the units against oracle/sam.py's decoder."""
import functools

import pytest
import torch

from oracle import sam as osam
from tests import decoder_reference as dr


@functools.lru_cache(maxsize=None)
def _w():
    return dr.weights(dr.build_decoder())


CASES = dr.all_cases(_w())


def _round(t, bf16):
    return t.to(dr.BF16) if bf16 else t


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_emulation_inside_mutants_outside(case):
    """4 R_order <= M <= R_mutant / 4 on this input set, and the emulation (rounded where the ABI rounds) inside the tolerance itself"""
    w, M = _w(), dr.M[case.unit]
    ref, emu = case.fn(dr.Arith(), w), case.fn(dr.Arith(emulate=True), w)
    for k, (r, tol) in case.reference(w).items():
        worst, share = dr.check(_round(emu[k], k in case.bf16), r, tol)
        assert worst <= 1.0, (k, worst, share)
    for order in (1, 2, 3):
        alt = case.fn(dr.Arith(emulate=True, order=order), w)
        for k in ref:
            r_order = dr.row_ratio(alt[k], ref[k], emu[k]).max().item()
            assert 4 * r_order <= M, (k, order, r_order)
            assert dr.check(_round(alt[k], k in case.bf16), ref[k], dr.tolerance(case.unit, ref[k], emu[k], k in case.bf16))[0] <= 1.0
    for mutant, outs in case.mutants.items():
        assert case.unit in dr.MUTANTS[mutant][0]
        alt = case.fn(dr.Arith(mutant=mutant), w)
        r_mutant = min(dr.row_ratio(alt[k], ref[k], emu[k]).min().item() for k in outs)
        assert r_mutant >= 4 * M, (mutant, r_mutant)
        for k in outs:         # and through the check the GPU file applies: every row of the judged outputs beyond the tolerance
            tol = dr.tolerance(case.unit, ref[k], emu[k], k in case.bf16)
            beyond = ((_round(alt[k], k in case.bf16).double() - ref[k]).abs() > tol).flatten(0, -2).any(-1)
            assert beyond.all(), (mutant, k, beyond.double().mean().item())


def test_every_mutant_is_used():
    used = {m for c in CASES for m in c.mutants}
    assert used == set(dr.MUTANTS)


def test_i2t_second_trip_case_emulation_inside():
    """the GPU file's case past the first trip of the persistent loop, as a 256-CU part gets it: P = 33 at hw = 1040"""
    P = dr.i2t_loop_prompts(256)
    assert P == 33 and 0 < P * 1040 - 128 * 256 < 128 * 256
    case = dr.i2t_case(P, 1040, "shared", True)
    emu = case.fn(dr.Arith(emulate=True), _w())
    r, tol = case.reference(_w())["keys"]
    assert dr.check(emu["keys"].to(dr.BF16), r, tol)[0] <= 1.0


def test_merge_partials_of_exact_partials_is_the_softmax():
    for hw, kind in ((48, "random"), (1040, "opposed"), (2304, "random")):
        q, kv = dr.attn_inputs(2, hw, kind, 7)
        part = dr.attn_partials(q, kv)
        assert part.shape == (2, 8, (hw + 1023) // 1024, dr.PART) and part.dtype == torch.float64
        ref = dr.attn_partial_reference(dr.Arith(), q, kv)
        assert (dr.merge_partials(part) - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()
        n = torch.tensor([min(1024, hw - s) for s in range(0, hw, 1024)], dtype=torch.float64)
        zero = dr.attn_partials(torch.zeros_like(q), kv)
        assert torch.equal(zero[..., 6:12], n.reshape(1, 1, -1, 1).expand(2, 8, -1, 6))         # l_s = the keys of the split when q = 0
    q, kv = dr.attn_inputs(3, 48, "random", 9, n_img=1)
    pimg = torch.zeros(3, dtype=torch.int32)
    assert torch.equal(dr.attn_partials(q, kv), dr.attn_partials(q, kv.expand(3, -1, -1), None))
    assert torch.equal(dr.attn_partials(q, kv), dr.attn_partials(q, kv, pimg))


def test_float64_chain_of_the_units_is_the_oracle_decoder():
    """two blocks plus the tail at the 5 + 1 token geometry: the per-stage references ARE the decoder (transformer.py:62-106,
    mask_decoder.py:116-164), not a private restatement of the kernels"""
    w, A = _w(), dr.Arith()
    P, h, wd = 2, 4, 8
    hw = h * wd
    src, pos = dr.rand((1, 256, h, wd), 1).double(), dr.rand((1, 256, h, wd), 2).double()
    sparse = dr.rand((P, 1, 256), 3).double()
    keys = src.flatten(2).permute(0, 2, 1).expand(P, -1, -1)
    kpe = pos.flatten(2).permute(0, 2, 1)
    lin = lambda x, name: x @ w[name + ".weight"].T + w[name + ".bias"]     # noqa: E731

    def kv_of(t2i, keys):
        k, v = lin(keys + kpe, t2i + ".k_proj"), lin(keys, t2i + ".v_proj")
        return torch.stack([k.reshape(P, hw, 8, 16), v.reshape(P, hw, 8, 16)], 3).reshape(P, hw, 256)

    def attend(q, t2i, keys):          # (float64 image rows: the bf16 cast of the kernel ABI is not part of the statement)
        kv = kv_of(t2i, keys).reshape(P, hw, 8, 2, 16)
        K, V = kv[:, :, :, 0].transpose(1, 2), kv[:, :, :, 1].transpose(1, 2)
        o = torch.softmax(dr._heads(q, 8) @ K.transpose(2, 3) / 4.0, -1) @ V
        return o.transpose(1, 2).reshape(P, 6, 128)

    blocks = [dr.L0, dr.L1]
    x = pe = part = None
    for i, blk in enumerate(blocks + [None]):
        t2i = blk + dr.T2I if blk else dr.FINAL
        norm = blk + ".norm2" if blk else dr.TR + ".norm_final_attn"
        stages = (dr.TOK_SELF if blk else 0) | dr.TOK_Q_T2I | (dr.TOK_INIT if i == 0 else dr.TOK_SUM_MLP)
        t = dr.tokens_reference(A, w, stages, i == 0, queries=x, query_pe=pe, self_blk=blk, t2i=t2i, norm=norm, sum_blk=blocks[i - 1] if i else None,
                                init_tokens=dr.init_tokens(w).double(), init_prompt=sparse[:, 0], mlp_part=part)
        x, pe = t["queries"], t["query_pe"]
        if i:
            prev = blocks[i - 1]
            keys = dr.i2t_rows_reference(A, w, prev, lin(keys + kpe, prev + ".cross_attn_image_to_token.q_proj"), t["k_i2t"], t["v_i2t"], keys)
        o = attend(t["q_t2i"], t2i, keys)
        x = dr.tokens_reference(A, w, dr.TOK_COMBINE, False, queries=x, query_pe=pe, t2i=t2i, norm=norm, attn_o=o)["queries"]
        if blk:
            part = dr.mlp_partial_reference(A, w, blk, x, 16)["partials"]
    heads = dr.heads_reference(A, w, x)
    masks = dr.upscale_reference(A, w, keys, heads["hyper"], h, wd, 0, 4)

    tokens = torch.cat([dr.init_tokens(w).double()[None].expand(P, -1, -1), sparse], 1)
    q_ref, k_ref = osam.two_way_transformer(w, dr.TR, src.expand(P, -1, -1, -1), pos.expand(P, -1, -1, -1), tokens)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()     # noqa: E731
    assert rel(x, q_ref) <= 1e-12 and rel(keys, k_ref) <= 1e-12
    m1, i1 = osam.mask_decoder(w, src, pos, sparse, torch.zeros(P, 256, h, wd, dtype=torch.float64), multimask_output=False, prefix="md")
    m3, i3 = osam.mask_decoder(w, src, pos, sparse, torch.zeros(P, 256, h, wd, dtype=torch.float64), multimask_output=True, prefix="md")
    assert rel(masks[:, :1], m1) <= 1e-12 and rel(masks[:, 1:], m3) <= 1e-12
    assert rel(heads["iou"][:, :1], i1) <= 1e-12 and rel(heads["iou"][:, 1:], i3) <= 1e-12
