"""The mask-decoder kernels of walkgpt_amd/csrc/decoder.hip, one by one, against the float64 references of tests/decoder_reference.py:
exact cases (operands chosen so that every intermediate fits what the kernel keeps: 16 bits at a bf16 hi + lo staging, 24 in an fp32
accumulator -- and needs both halves of the pair), tolerance cases (M * E_row, formed on the reference side only) and the host's refusals.
Every output carries one guard prompt (row P) and is pre-filled with a poison value: the guard must come back untouched and no poison may
be left inside.  The kernel operands come from the module's own helpers (token_stage_table, _tiled, head_weights, _convt_as_gemm,
_build_prepared), so the host re-layouts are under test as well; the references read the plain state_dict tensors."""
import ctypes
import functools

import pytest
import torch

from tests import decoder_reference as dr
from walkgpt_amd import _lib, ops
from walkgpt_amd.segment_anything import modeling as M

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
POISON = -24680.0           # (bf16-representable: the same bits in both output types)


def _report(what, worst, share):
    print("decoder tolerance: %s  worst %.3f of the tolerance, %.4f of the elements beyond it" % (what, worst, share))
    assert worst <= 1.0, "%s: %.2f x the tolerance, %.2f %% of the elements beyond it" % (what, worst, 100 * share)


def _report_case(case, refs, outs):
    for k, (ref, tol) in refs.items():
        _report("%r %s" % (case, k), *dr.check(outs[k], ref, tol))


# ---- guard rows and poison -------------------------------------------------------------------------------------------------------------------
def _guarded(dev, P, *rest, dtype=torch.float32):
    """-> (the [P, ...] view a kernel writes, the [P + 1, ...] buffer behind it, poisoned)"""
    full = torch.full((P + 1,) + tuple(rest), POISON, device=dev, dtype=dtype)
    return full[:P], full


def _intact(*fulls, inputs=()):
    """the guard prompt untouched, no poison left inside (`inputs`: buffers whose inside the kernel only reads or updates)"""
    for full in fulls + tuple(inputs):
        assert bool((full[-1] == POISON).all()), "guard row written"
    for full in fulls:
        assert not bool((full[:-1] == POISON).any()) and bool(torch.isfinite(full[:-1].float()).all()), "output not fully written"


class _Guard:
    """The ops.* wrappers allocate their outputs themselves (torch.empty / empty_like): inside this context each such buffer gets a guard
    prompt and the poison; `intact()` afterwards."""

    def __enter__(self):
        self.fulls, self._empty, self._like = [], torch.empty, torch.empty_like
        torch.empty, torch.empty_like = self._alloc, lambda t: self._alloc(*t.shape, device=t.device, dtype=t.dtype)
        return self

    def _alloc(self, *shape, **kw):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        full = self._empty(shape[0] + 1, *shape[1:], **kw).fill_(POISON)
        self.fulls.append(full)
        return full[:shape[0]]

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self._empty, self._like

    def intact(self):
        assert self.fulls
        _intact(*self.fulls)


# ---- the module and its operands -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoder(dev):
    dec = dr.build_decoder().to(dev)
    return dec, dr.weights(dec)


def _mod(dec, prefix):
    return None if prefix is None else dec.get_submodule(prefix[3:])


def _table(dec, ins):
    return M.token_stage_table(self_blk=_mod(dec, ins.get("self_blk")), t2i=_mod(dec, ins.get("t2i")), norm=_mod(dec, ins.get("norm")),
                               sum_blk=_mod(dec, ins.get("sum_blk")))


def _combine(dec, part, t2i=dr.FINAL, norm=dr.TR + ".norm_final_attn"):
    a, n = _mod(dec, t2i), _mod(dec, norm)
    return (part, M._tiled(a.out_proj.weight), a.out_proj.bias, n.weight, n.bias)


def _run_tokens(dev, stages, skip_pe, table, P, queries=None, query_pe=None, init_tokens=None, init_prompt=None, attn_part=None, mlp_part=None,
                prompt_tail=None):
    """ops.dec_tokens on guarded, poisoned buffers -> dict of the outputs the stages write (CPU) after the guard / poison checks"""
    g = lambda t: None if t is None else t.to(dev).contiguous()      # noqa: E731
    q, qf = _guarded(dev, P, 6, 256)
    pe, pef = _guarded(dev, P, 6, 256)
    init = bool(stages & ops.TOK_INIT)
    if not init:
        q.copy_(queries)
        pe.copy_(query_pe)
    qt, qtf = _guarded(dev, P, 6, 128)
    ki, kif = _guarded(dev, P, 6, 128, dtype=BF16)
    vi, vif = _guarded(dev, P, 6, 128, dtype=BF16)
    ops.dec_tokens(stages, skip_pe, q, pe, table, q_t2i=qt if stages & ops.TOK_Q_T2I else None, attn_partials=g(attn_part), mlp_partials=g(mlp_part),
                   k_i2t=ki if stages & ops.TOK_SUM_MLP else None, v_i2t=vi if stages & ops.TOK_SUM_MLP else None,
                   init_tokens=g(init_tokens), init_prompt=g(init_prompt), prompt_tail=prompt_tail)
    torch.cuda.synchronize()
    written = [qf, pef] + ([qtf] if stages & ops.TOK_Q_T2I else []) + ([kif, vif] if stages & ops.TOK_SUM_MLP else [])
    _intact(*written)
    for full in (qtf, kif, vif):
        if not any(full is f for f in written):
            assert bool((full == POISON).all()), "an output of a stage that did not run was written"
    return dict(queries=q.cpu(), query_pe=pe.cpu(), q_t2i=qt.cpu(), k_i2t=ki.cpu(), v_i2t=vi.cpu())


# =====================================================================================================================================
# exact cases
# =====================================================================================================================================
def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _frac_rows(shape, bits, seed):
    """n + m 2^-bits, |n| <= 3, 0 < m < 2^bits: 2 + bits significant bits, more than the 8 of one bf16 -- both halves of the pair are needed"""
    x = _ints(shape, -3, 3, seed) + _ints(shape, 1, 2 ** bits - 1, seed + 1) * 2.0 ** -bits
    assert not torch.equal(x.float().to(BF16).double(), x)
    return x


def _sparse_ints(n, k, nnz, seed):
    """[n, k] with nnz nonzeros per row: +-1 and one +-2 (asymmetric: no two columns or rows play the same part)"""
    g = torch.Generator().manual_seed(seed)
    wt = torch.zeros(n, k, dtype=torch.float64)
    for r in range(n):
        cols = torch.randperm(k, generator=g)[:nnz]
        wt[r, cols] = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).double()
        wt[r, cols[0]] *= 2
    return wt


def _tile(dev, wt, k_slices=1):
    return ops.tile_weight(wt.to(dev, BF16).contiguous(), k_slices)


@pytest.mark.parametrize("P", [1, 5])
def test_exact_q_t2i(dev, P):
    """Q_T2I alone is a bare fp32 Linear: q_t2i = W_q (x + pe) + b.  x integer, pe = m 2^-10: x + pe has 12 significant bits; weights in
    -2 .. 2: the sums stay below 2^11 at a resolution of 2^-10, 21 bits."""
    x, pe = _ints((P, 6, 256), -3, 3, 11), _ints((P, 6, 256), 1, 1023, 12) * 2.0 ** -10
    wq, bq = _ints((128, 256), -2, 2, 13), _ints((128,), -5, 5, 14)
    table = [None] * 24
    table[10:12] = [_tile(dev, wq), bq.to(dev, BF16)]
    out = _run_tokens(dev, ops.TOK_Q_T2I, False, table, P, queries=x.float(), query_pe=pe.float())
    ref = (x + pe) @ wq.T + bq
    assert torch.equal(out["q_t2i"].double(), ref)
    assert torch.equal(out["queries"].double(), x) and torch.equal(out["query_pe"].double(), pe)


@pytest.mark.parametrize("P", [1, 5])
def test_exact_init(dev, P):
    """INIT: queries == query_pe == cat(init_tokens, prompt) bit for bit (mask_decoder.py:125-132), and the q projection behind it"""
    tokens = dr.rand((5, 256), 21)
    prompt = (_ints((P, 256), -3, 3, 22) + _ints((P, 256), 1, 31, 23) / 32).to(BF16)
    ref = torch.cat([tokens[None].expand(P, -1, -1), prompt.float()[:, None]], 1)
    out = _run_tokens(dev, ops.TOK_INIT, False, [None] * 24, P, init_tokens=tokens, init_prompt=prompt)
    assert torch.equal(out["queries"], ref) and torch.equal(out["query_pe"], ref)


@pytest.mark.parametrize("P", [1, 5])
def test_exact_init_through_prompt_tail(dev, P):
    """wg_dec_tokens_ctp_f32: the same bits as ops.ctp_tail followed by the plain launch, as the header promises"""
    dec, w = _decoder(dev)
    ins = dict(self_blk=dr.L0, t2i=dr.L0 + dr.T2I, norm=dr.L0 + ".norm2")
    table = _table(dec, ins)
    tokens = dr.init_tokens(w)
    pre = dr.rand_bf16((P, 256), 31, 2.0)
    g_, b_, tt_ = (1 + dr.rand((256,), 32, 0.2)).to(BF16), dr.rand_bf16((256,), 33, 0.1), dr.rand_bf16((256,), 34, 0.5)
    lt_ = torch.tensor([0.75], dtype=BF16)
    tail = tuple(t.to(dev) for t in (g_, b_, tt_, lt_)) + (1e-5,)
    stages = ops.TOK_INIT | ops.TOK_SELF | ops.TOK_Q_T2I
    with _Guard() as guard:
        row = ops.ctp_tail(pre.to(dev), *tail)
    torch.cuda.synchronize()
    guard.intact()
    two = _run_tokens(dev, stages, True, table, P, init_tokens=tokens, init_prompt=row)
    one = _run_tokens(dev, stages, True, table, P, init_tokens=tokens, init_prompt=pre, prompt_tail=tail)
    for k in ("queries", "query_pe", "q_t2i"):
        assert torch.equal(one[k], two[k]), k
    A = dr.Arith(emulate=True)
    ref = dr.ctp_tail_reference(dr.Arith(), pre, g_, b_, tt_, lt_, 1e-5)
    tol = dr.tolerance("tokens", ref, dr.ctp_tail_reference(A, pre, g_, b_, tt_, lt_, 1e-5), True)
    _report("ctp tail row P%d" % P, *dr.check(one["query_pe"][:, 5], ref, tol))


@pytest.mark.parametrize("P", [1, 5])
def test_exact_mlp_partial(dev, P):
    """x = n + m 2^-10 (12 bits); lin1 with four nonzeros a row (+-1, one +-2) and an integer bias: the hidden values stay below 32 at a
    resolution of 2^-10, 15 bits <= 16; lin2 in -1 .. 1 over the 128 units of a slice: below 2^12, 22 bits <= 24"""
    S = ops.dec_mlp_slices()
    x = _frac_rows((P, 6, 256), 10, 41)
    w1, b1, w2 = _sparse_ints(2048, 256, 4, 43), _ints((2048,), -3, 3, 44), _ints((256, 2048), -1, 1, 45)
    hid = torch.relu(x @ w1.T + b1)
    assert hid.abs().max() < 32 and not torch.equal(hid.float().to(BF16).double(), hid)
    n = 2048 // S
    ref = torch.stack([hid[..., s * n:(s + 1) * n] @ w2[:, s * n:(s + 1) * n].T for s in range(S)], 1)
    ops_in = (x.float().to(dev), _tile(dev, w1), b1.to(dev, BF16), _tile(dev, w2, S))
    with _Guard() as guard:
        out = ops.dec_mlp_partial(*ops_in)
    torch.cuda.synchronize()
    guard.intact()
    assert out.shape == (P, S, 6, 256) and torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("P", [1, 5])
def test_exact_heads(dev, P):
    """x = n + m 2^-8 (10 bits); three sparse small-integer layers: |h0| <= 20 + 3 (13 bits), |h1| <= 5 * 23 + 3 (15 bits), the last sums
    below 2^11 at 2^-8 (19 bits)"""
    x = _frac_rows((P, 6, 256), 8, 51)
    layers, weights = [], []
    for i in range(5):
        n_out = 32 if i < 4 else 4
        ws = [(_sparse_ints(256, 256, 4, 60 + 10 * i), _ints((256,), -3, 3, 61 + 10 * i)),
              (_sparse_ints(256, 256, 4, 62 + 10 * i), _ints((256,), -3, 3, 63 + 10 * i)),
              (_sparse_ints(n_out, 256, 8, 64 + 10 * i), _ints((n_out,), -3, 3, 65 + 10 * i))]
        layers.append(ws)
        for wt, b in ws:
            weights += [_tile(dev, wt), b.to(dev, BF16)]

    def mlp(i, row):
        h = row
        for j, (wt, b) in enumerate(layers[i]):
            h = h @ wt.T + b
            if j < 2:
                h = torch.relu(h)
                assert h.abs().max() < (32, 128)[j]
        return h

    hyper_ref = torch.stack([mlp(i, x[:, 1 + i]) for i in range(4)], 1)
    iou_ref = mlp(4, x[:, 0])
    xd = x.float().to(dev)
    with _Guard() as guard:
        hyper, iou = ops.dec_heads(xd, weights)
    torch.cuda.synchronize()
    guard.intact()
    assert torch.equal(hyper.cpu().double(), hyper_ref) and torch.equal(iou.cpu().double(), iou_ref)


EXACT_HW = (1, 16, 48, 240, 256, 272, 1000, 1024, 1025, 1040, 2304, 4096)


@pytest.mark.parametrize("form", ["prompt", "shared", "map"])
@pytest.mark.parametrize("P", [1, 3])
def test_exact_attn_partial_counts_every_key_once(dev, P, form):
    """q = 0, integer V (|v| <= 3): every score is 0, every weight exactly 1, so for every split l_s is the number of its keys, their sum is
    hw, and the o_s add up to the integer column sums of V: every key counted once and none past hw.  kv_img is a column slice of a wider
    buffer (as proj[..., :256] is) whose other columns and trailing guard rows are NaN: nothing may leak."""
    n_img = {"prompt": P, "shared": 1, "map": 2}[form]
    pimg = torch.tensor([(p + 1) % 2 for p in range(P)], dtype=torch.int32) if form == "map" else None
    q = torch.zeros(P, 6, 128, device=dev)
    for hw in EXACT_HW:
        v = _ints((n_img, hw, 8, 16), -3, 3, 70 + hw)
        k = dr.rand((n_img, hw, 8, 16), 71 + hw).double()
        buf = torch.full((n_img, hw + 2, 384), float("nan"), device=dev, dtype=BF16)
        buf[:, :hw, :256] = torch.stack([k, v], 3).reshape(n_img, hw, 256).to(dev, BF16)
        with _Guard() as guard:
            part = ops.dec_attn_partial(q, buf[:, :hw, :256], None if pimg is None else pimg.to(dev))
        torch.cuda.synchronize()
        guard.intact()
        S = (hw + 1023) // 1024
        assert part.shape == (P, 8, S, dr.PART)
        part = part.cpu().double()
        counts = torch.tensor([min(1024, hw - 1024 * s) for s in range(S)], dtype=torch.float64)
        assert torch.equal(part[..., :6], torch.zeros(P, 8, S, 6, dtype=torch.float64)), hw
        assert torch.equal(part[..., 6:12], counts.reshape(1, 1, S, 1).expand(P, 8, S, 6)), hw
        assert part[..., 6:12].sum(2).eq(hw).all()
        vsel = v if form == "prompt" else v[pimg.long()] if form == "map" else v.expand(P, -1, -1, -1)
        colsum = vsel.sum(1)                                                        # [P, 8, 16]
        assert torch.equal(part[..., 12:].reshape(P, 8, S, 6, 16).sum(2), colsum[:, :, None].expand(P, 8, 6, 16)), hw
        merged = dr.merge_partials(part)                                            # [P, 6, 128]
        assert torch.equal(merged, (colsum / hw).reshape(P, 1, 128).expand(P, 6, 128)), hw


# =====================================================================================================================================
# tolerance cases
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _token_cases(dev):
    _, w = _decoder(dev)
    return {repr(c): c for P in (1, 5) for c in dr.tokens_cases(w, P)}


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("name", ["init_self_q", "sum_self_q", "sum_q", "self_q", "combine", "sum"])
def test_tokens(dev, name, P):
    """wg_dec_tokens_f32 for each stage mask the chain issues, each on its own inputs"""
    dec, w = _decoder(dev)
    case = _token_cases(dev)["tokens:%s_P%d" % (name, P)]
    ins = case.inputs
    out = _run_tokens(dev, ins["stages"], ins["skip_pe"], _table(dec, ins), P, queries=ins.get("queries"), query_pe=ins.get("query_pe"),
                      init_tokens=ins.get("init_tokens"), init_prompt=ins.get("init_prompt"), attn_part=ins.get("attn_part"),
                      mlp_part=ins.get("mlp_part"))
    _report_case(case, case.reference(w), out)
    if not ins["stages"] & ops.TOK_INIT:
        assert torch.equal(out["query_pe"], ins["query_pe"])


@pytest.mark.parametrize("idx", range(5))
def test_attn_partial(dev, idx):
    """wg_dec_attn_partial_f32 -> float64 merge of its partials against the softmax over all hw keys"""
    case = dr.attn_cases()[idx]
    with _Guard() as guard:
        part = ops.dec_attn_partial(case.inputs["q"].to(dev), case.inputs["kv"].to(dev))
    torch.cuda.synchronize()
    guard.intact()
    if "opposed" in case.name:
        m = part[..., :6].cpu()
        print("per-split maxima differ by %.1f .. %.1f" % ((m[:, :, 0] - m[:, :, 1]).min().item(), (m[:, :, 0] - m[:, :, 1]).max().item()))
        assert (m[:, :, 0] - m[:, :, 1]).min() > 50
    _report_case(case, case.reference(None), {"o": dr.merge_partials(part.cpu())})


def test_attn_partials_through_the_three_combine_consumers(dev):
    """the same GPU partials (per-split maxima about 100 apart: a merge without the rescale fails) through dec_tokens(COMBINE),
    dec_mlp_partial(combine=) with its x_out, and dec_heads(combine=)"""
    dec, w = _decoder(dev)
    c_tok, c_mlp, c_heads = dr.chain_cases(w)
    ins = c_tok.inputs
    P = ins["q"].shape[0]
    x, pe = ins["queries"], ins["query_pe"]
    part = ops.dec_attn_partial(ins["q"].to(dev), ins["kv"].to(dev))
    out = _run_tokens(dev, ops.TOK_COMBINE, False, _table(dec, ins), P, queries=x, query_pe=pe, attn_part=part)
    _report_case(c_tok, c_tok.reference(w), out)
    comb = _combine(dec, part)
    blk = _mod(dec, dr.L1)
    lin = (M._tiled(blk.mlp.lin1.weight), blk.mlp.lin1.bias, M._tiled(blk.mlp.lin2.weight, ops.dec_mlp_slices()))
    heads_w = dec.head_weights()
    xd = x.to(dev)
    with _Guard() as guard:
        mlp, x_out = ops.dec_mlp_partial(xd, *lin, combine=comb)
        hyper, iou = ops.dec_heads(xd, heads_w, combine=comb)
    torch.cuda.synchronize()
    guard.intact()
    assert torch.equal(x_out.cpu(), out["queries"])          # both run the same tok_combine
    assert torch.equal(xd.cpu(), x)
    b2 = w[dr.L1 + ".mlp.lin2.bias"]
    _report_case(c_mlp, c_mlp.reference(w), {"partials": mlp.cpu(), "sum": mlp.cpu().double().sum(1) + b2})
    _report_case(c_heads, c_heads.reference(w), {"hyper": hyper.cpu(), "iou": iou.cpu()})


@pytest.mark.parametrize("P", [1, 5])
def test_mlp_partial(dev, P):
    dec, w = _decoder(dev)
    case, = dr.mlp_cases(P)
    blk = _mod(dec, case.inputs["blk"])
    with _Guard() as guard:
        out = ops.dec_mlp_partial(case.inputs["x"].to(dev), M._tiled(blk.mlp.lin1.weight), blk.mlp.lin1.bias,
                                  M._tiled(blk.mlp.lin2.weight, ops.dec_mlp_slices()))
    torch.cuda.synchronize()
    guard.intact()
    total = out.cpu().double().sum(1) + w[case.inputs["blk"] + ".mlp.lin2.bias"]
    _report_case(case, case.reference(w), {"partials": out.cpu(), "sum": total})


@pytest.mark.parametrize("P", [1, 5])
def test_heads(dev, P):
    dec, w = _decoder(dev)
    case, = dr.heads_cases(P)
    heads_w = dec.head_weights()
    with _Guard() as guard:
        hyper, iou = ops.dec_heads(case.inputs["x"].to(dev), heads_w)
    torch.cuda.synchronize()
    guard.intact()
    _report_case(case, case.reference(w), {"hyper": hyper.cpu(), "iou": iou.cpu()})


def _run_i2t(dev, case):
    dec, w = _decoder(dev)
    ins = case.inputs
    blk = _mod(dec, ins["blk"])
    i2t = blk.cross_attn_image_to_token
    g = lambda t: None if t is None else t.to(dev)      # noqa: E731
    proj = torch.full(ins["q_img"].shape[:2] + (384,), float("nan"), device=dev, dtype=BF16)      # q is a column slice of the image-side projection
    proj[..., 256:] = ins["q_img"].to(dev)
    with _Guard() as guard:
        out = ops.dec_i2t_rows(proj[..., 256:], g(ins["k_i2t"]), g(ins["v_i2t"]), i2t.out_proj.weight, i2t.out_proj.bias, g(ins["keys"]),
                               blk.norm4.weight, blk.norm4.bias, blk.norm4.eps, ins["P"], res_bias=g(ins["res_bias"]),
                               prompt_image=g(ins["prompt_image"]))
    torch.cuda.synchronize()
    guard.intact()
    _report_case(case, case.reference(w), {"keys": out.cpu()})


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("form", ["prompt", "shared", "map"])
@pytest.mark.parametrize("P,hw", dr.I2T_SHAPES)
def test_i2t_rows(dev, P, hw, form, bias):
    _run_i2t(dev, dr.i2t_case(P, hw, form, bias))


def test_i2t_rows_second_trip_of_the_persistent_loop(dev):
    """more rows than one trip of the grid (128 rows per workgroup, one workgroup per CU), the last trip partly filled"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    P = dr.i2t_loop_prompts(cus)
    over = P * 1040 - 128 * cus
    print("CUs %d, P %d: %d rows, %d past the first trip" % (cus, P, P * 1040, over))
    assert 0 < over < 128 * cus
    _run_i2t(dev, dr.i2t_case(P, 1040, "shared", True))


@functools.lru_cache(maxsize=None)
def _upscale_reference(dev, shape):
    _, w = _decoder(dev)
    case = dr.upscale_case(*shape)
    return case, case.reference(w)["masks"]


@pytest.mark.parametrize("first,num", dr.UPSCALE_MASKS)
@pytest.mark.parametrize("shape", dr.UPSCALE_SHAPES, ids=lambda s: "P%d_%dx%d" % s)
def test_upscale_mask(dev, shape, first, num):
    """wg_upscale_mask_bf16: w % 16 != 0 (a 16-token group spans image lines), and 768 groups on the 512-block grid at (3, 64, 64)"""
    dec, w = _decoder(dev)
    case, (ref, tol) = _upscale_reference(dev, shape)
    P, h, wd = shape
    p = dec._build_prepared()
    up, ln1 = dec.output_upscaling, dec.output_upscaling[1]
    keys, hyper = case.inputs["keys"].to(dev), case.inputs["hyper"].to(dev)
    with _Guard() as guard:
        out = ops.upscale_mask(keys, p["up1_w"], up[0].bias, ln1.weight, ln1.bias, ln1.eps, p["up2_w"], up[3].bias, hyper, h, wd, first, num)
    torch.cuda.synchronize()
    guard.intact()
    assert out.shape == (P, num, 4 * h, 4 * wd)
    _report("%r masks %d..%d" % (case, first, first + num - 1), *dr.check(out, ref[:, first:first + num], tol[:, first:first + num]))


# =====================================================================================================================================
# refusals: WG_REQUIRE on the host, before any launch
# =====================================================================================================================================
def _refused(rc, word):
    msg = _lib.lib().wg_last_error().decode()
    assert rc != 0 and word in msg, (rc, msg)


def test_refusals(dev):
    dec, _ = _decoder(dev)
    L = _lib.lib()
    P = 2
    f32 = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    bf = lambda *s: torch.zeros(*s, device=dev, dtype=BF16)      # noqa: E731
    q, pe, qt, ki, vi = f32(P, 6, 256), f32(P, 6, 256), f32(P, 6, 128), bf(P, 6, 128), bf(P, 6, 128)
    mlp_part, tokens, prompt = f32(P, ops.dec_mlp_slices(), 6, 256), f32(5, 256), bf(P, 256)
    blk = _mod(dec, dr.L0)
    tab = M.token_stage_table(self_blk=blk, t2i=blk.cross_attn_token_to_image, norm=blk.norm2, sum_blk=blk)
    ctab = (ctypes.c_void_p * 24)(*[None if t is None else t.data_ptr() for t in tab])
    rc = L.wg_dec_tokens_f32(ops.TOK_INIT | ops.TOK_SUM_MLP, 0, q.data_ptr(), pe.data_ptr(), tokens.data_ptr(), prompt.data_ptr(), ctab, 24,
                             qt.data_ptr(), None, 0, mlp_part.data_ptr(), ki.data_ptr(), vi.data_ptr(), P, 1e-5, None)
    _refused(rc, "INIT")
    hw = 1040
    kv = bf(P, hw, 256)
    for n_splits in (1, 3):
        part = f32(P, 8, 3, dr.PART)
        rc = L.wg_dec_attn_partial_f32(qt.data_ptr(), kv.data_ptr(), kv.data_ptr() + 32, 256, 32, hw, None, hw, part.data_ptr(), n_splits, P, None)
        _refused(rc, "n_splits")
    part = f32(P, 8, 2, dr.PART)
    comb = _combine(dec, part)
    cc = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in comb])
    out = f32(P, ops.dec_mlp_slices(), 6, 256)
    lin = (M._tiled(blk.mlp.lin1.weight), blk.mlp.lin1.bias, M._tiled(blk.mlp.lin2.weight, ops.dec_mlp_slices()))
    rc = L.wg_dec_mlp_partial_f32(q.data_ptr(), cc, 2, 1e-5, q.data_ptr(), lin[0].data_ptr(), lin[1].data_ptr(), lin[2].data_ptr(), out.data_ptr(), P, None)
    _refused(rc, "x_out")
    i2t = blk.cross_attn_image_to_token
    with pytest.raises(_lib.WalkgptHipError, match="multiple of 16"):
        ops.dec_i2t_rows(bf(P, 24, 128), ki, vi, i2t.out_proj.weight, i2t.out_proj.bias, bf(P, 24, 256), blk.norm4.weight, blk.norm4.bias, 1e-5, P)
    torch.cuda.synchronize()
    assert float(q.abs().sum()) == 0 and float(out.abs().sum()) == 0          # nothing was launched
