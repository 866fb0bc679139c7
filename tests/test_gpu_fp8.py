"""fp8 (OCP e4m3) GEMM path of BASELINE config C5: operand layout of the block-scaled MFMA on exact integer data, the row quantiser
against torch's float8_e4m3fn, the GEMM against fp32 on the dequantised operands, and what the path costs in parity: encoder output and
thresholded masks against the same references as the bf16 path, with the measured deltas printed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden import cases
from tests.test_gpu_modules import build_encoder, rel_err
from walkgpt_amd import ops

F8 = torch.float8_e4m3fn


def _q(t):
    return t.to(F8).view(torch.uint8).contiguous()


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 264, 384), (1000, 520, 1280)])
def test_fp8_gemm_exact_on_small_integers(dev, M, N, K):
    """Integers in [-3, 3] are exact in e4m3 and their products sum exactly in fp32: any error in the fragment layout (which 32 bytes of
    a row belong to which lane of v_mfma_scale_f32_16x16x128_f8f6f4) shows up as a wrong integer.  Asymmetric operands."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-3, 4, (N, K), generator=g).float()
    w[:, ::7] = 0.0
    sa = (torch.arange(M) % 5 + 1).float()                 # per-row / per-channel scales that are exact too
    sw = (torch.arange(N) % 3 + 1).float() * 0.5
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    out = ops.linear_fp8(_q(a).to(dev), sa.to(dev), _q(w).to(dev), sw.to(dev), bias=bias.to(dev, torch.bfloat16))
    ref = (a @ w.t()) * sa[:, None] * sw[None, :] + bias
    got = out.float().cpu()
    exact = ref.to(torch.bfloat16).float()                 # the only rounding left is the bf16 output
    assert torch.equal(got, exact), float((got - exact).abs().max())


def test_quantize_rows_matches_float8_e4m3fn(dev):
    x = (torch.randn(77, 1280, generator=torch.Generator().manual_seed(3)) * 3).to(torch.bfloat16)
    x[5] = 0
    q, s = ops.quantize_rows_fp8(x.to(dev))
    amax = x.float().abs().amax(1)
    s_ref = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.allclose(s.cpu(), s_ref, rtol=1e-6)
    q_ref = _q(x.float() / s_ref[:, None])
    same = (q.cpu() == q_ref).float().mean().item()
    assert same > 0.995, same                              # (ties of the two divisions may round differently: reciprocal-multiply here)
    deq = q.cpu().view(F8).float() * s.cpu()[:, None]
    assert rel_err(deq.numpy(), x.float().numpy()) < 0.04
    # LayerNorm fused in front: against torch's LayerNorm followed by the same quantisation
    g_ = torch.randn(1280, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    b_ = torch.randn(1280, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    q2, s2 = ops.quantize_rows_fp8(x.to(dev), ln=(g_.to(dev), b_.to(dev)), eps=1e-6)
    y = torch.nn.functional.layer_norm(x.float(), (1280,), g_.float(), b_.float(), 1e-6)
    y[5] = b_.float()
    deq2 = q2.cpu().view(F8).float() * s2.cpu()[:, None]
    assert rel_err(deq2.numpy(), y.numpy()) < 0.04
    assert torch.allclose(s2.cpu(), y.abs().amax(1) / 448.0, rtol=2e-3)


@pytest.mark.parametrize("M,N,K,act", [(4096, 768, 768, 0), (1025, 3072, 768, 1), (8200, 1024, 4096, 0)])
def test_fp8_linear_vs_fp32_on_dequantised_operands(dev, M, N, K, act):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    r = torch.randn(M, N, generator=g).to(torch.bfloat16)
    xq, xs = ops.quantize_rows_fp8(x.to(dev))
    wq, ws = ops.quantize_weight_fp8(w.to(dev))
    out = ops.linear_fp8(xq, xs, wq, ws, bias=b.to(dev), act=act, residual=r.to(dev))
    xd = xq.cpu().view(F8).float() * xs.cpu()[:, None]
    wd = wq.cpu().view(F8).float() * ws.cpu()[:, None]
    y = xd @ wd.t() + b.float()
    if act == 1:
        y = torch.nn.functional.gelu(y)
    y = y + r.float()
    assert rel_err(out.float().cpu().numpy(), y.numpy()) < 4e-3          # same operands: only accumulation order + the bf16 output
    full = x.float() @ w.float().t() + b.float()
    if act == 1:
        full = torch.nn.functional.gelu(full)
    full = full + r.float()
    e = rel_err(out.float().cpu().numpy(), full.numpy())
    print("fp8 linear M=%d N=%d K=%d: rel err vs unquantised fp32 %.4f" % (M, N, K, e))
    assert e < 0.05


def _mx_reference(h):
    """OCP-MX quantisation of bf16 rows as the GEMM epilogue states it: per (row, 32 columns) the power of two at or above max / 448 (E8M0
    byte = exponent + 127), values divided by it and rounded to e4m3.  -> (bytes [M, N], scale bytes [N / 32, M])."""
    M, N = h.shape
    blk = h.float().view(M, N // 32, 32)
    am = blk.abs().amax(-1).clamp_min(2.0 ** -100)
    e = torch.ceil(torch.log2(am.double() / 448.0)).clamp(-127, 126)
    q = (blk / torch.exp2(e).float()[..., None]).to(F8).view(torch.uint8).view(M, N)
    return q, (e + 127).to(torch.uint8).t().contiguous()


def _mx_deq(q, mx, rows, group):
    """e4m3 bytes [rows, K] + block-scale planes -> fp32 values"""
    K = q.shape[1]
    e = mx[:, ops.mx_scale_index(rows, mx.device, group)].float() - 127.0          # [K/32, rows]
    return (q.view(F8).float().view(rows, K // 32, 32) * torch.exp2(e).t()[..., None]).view(rows, K)


@pytest.mark.parametrize("M,K,group", [(300, 128, 128), (4099, 768, 128), (520, 1280, 64)])
def test_quantize_mx_matches_the_stated_rule(dev, M, K, group):
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) * 3).to(torch.bfloat16)
    x[:, 32:64] *= 1e-3
    x[7] = 0
    q, mx = ops.quantize_mx_fp8(x.to(dev), group=group)
    q_ref, s_ref = _mx_reference(x)
    assert torch.equal(mx[:, ops.mx_scale_index(M, dev, group)].cpu(), s_ref)
    assert torch.equal(q.cpu(), q_ref)
    assert rel_err(_mx_deq(q, mx, M, group).cpu().numpy(), x.float().numpy()) < 0.04
    if K % 256 == 0:                                       # the chain-entry form: the same pass also leaves the rows' partial sums
        xd = x.to(dev)
        q2, mx2, part = ops.quantize_mx_fp8(xd, group=group, row_partials=True)
        idx = ops.mx_scale_index(M, dev, group)
        assert torch.equal(q2, q) and torch.equal(mx2[:, idx], mx[:, idx])
        part = part.cpu()[:, :M]
        tiles = x.float().view(M, K // 256, 256)
        assert torch.allclose(part[..., 0].t(), tiles.sum(-1), rtol=1e-5, atol=1e-3)
        assert torch.allclose(part[..., 1].t(), (tiles * tiles).sum(-1), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("B,window,heads", [(2, 14, 12), (1, 64, 12), (3, 14, 16), (2, 64, 16)])
def test_attention_writes_its_output_as_the_mx_operand(dev, B, window, heads):
    """fp8 chain, head_dim 64 (ViT-B / ViT-L): the SAM attention kernels write e4m3 bytes + block scales themselves -- bit for bit what
    wg_quantize_mx_fp8 makes of their bf16 output (the stated rule: test_quantize_mx_matches_the_stated_rule), scale bytes included, for the
    windowed kernel (padded windows at the image edge: 64 = 4 x 14 + 8) and the global one."""
    g = torch.Generator().manual_seed(B * 100 + window)
    grid, hd = 64, 64
    D = heads * hd
    M = B * grid * grid
    qkv = (torch.randn(M, 3 * D, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    qb = (torch.randn(3 * D, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    rh = (torch.randn(2 * window - 1, hd, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    rw = (torch.randn(2 * window - 1, hd, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    o = ops.sam_attention(qkv, qb, rh, rw, B, grid, window, heads)
    q_ref, mx_ref = ops.quantize_mx_fp8(o)
    got = ops.sam_attention(qkv, qb, rh, rw, B, grid, window, heads, mx_out=True)
    assert got.mx is not None and got.x is None, "head_dim 64 with window 14 / global 64 x 64 carries the MX epilogue"
    q, mx = got.mx
    idx = ops.mx_scale_index(M, dev, 128)
    assert torch.equal(mx[:, idx], mx_ref[:, idx])
    assert torch.equal(q, q_ref)


def test_attention_mx_epilogue_is_not_offered_at_head_dim_80(dev):
    """ViT-H: a 32-column block would straddle two heads; the caller gets bf16 and quantises in a pass of its own."""
    g = torch.Generator().manual_seed(1)
    B, grid, window, heads, hd = 1, 64, 14, 16, 80
    D = heads * hd
    qkv = torch.randn(B * grid * grid, 3 * D, generator=g).to(torch.bfloat16).to(dev)
    qb = torch.zeros(3 * D, dtype=torch.bfloat16, device=dev)
    rh = torch.zeros(2 * window - 1, hd, dtype=torch.bfloat16, device=dev)
    out = ops.sam_attention(qkv, qb, rh, rh.clone(), B, grid, window, heads, mx_out=True)
    assert out.mx is None and out.x.dtype == torch.bfloat16


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 264, 384), (1000, 520, 1280), (2100, 1032, 256)])
def test_mxfp8_persistent_gemm_exact_on_small_integers(dev, M, N, K):
    """Both operands with per-(row, block) power-of-two scales on exact integer data, on the persistent kernel (several tiles per
    workgroup at the larger shapes): a scale byte of either side that reaches the wrong row, K block, fragment or TILE changes an integer."""
    g = torch.Generator().manual_seed(M + N + K + 2)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-3, 4, (N, K), generator=g).float()
    w[:, ::5] = 0.0
    ea = torch.randint(-2, 3, (K // 32, M), generator=g)
    ew = torch.randint(-2, 3, (K // 32, N), generator=g)
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    res = torch.randint(-8, 9, (M, N), generator=g).float()
    pa = torch.full((K // 32, ops.mx_pitch(M)), 255, dtype=torch.uint8)              # rows past M / N: NaN scales, must never reach the output
    pa[:, ops.mx_scale_index(M)] = (ea + 127).to(torch.uint8)
    pw = torch.full((K // 32, ops.mx_pitch(N)), 255, dtype=torch.uint8)
    pw[:, ops.mx_scale_index(N, group=64)] = (ew + 127).to(torch.uint8)
    out = ops.linear_mxfp8((_q(a).to(dev), pa.to(dev)), {"q": _q(w).to(dev), "mx": pw.to(dev)}, bias=bias.to(dev, torch.bfloat16),
                           residual=res.to(dev, torch.bfloat16))
    a_deq = a * torch.exp2(ea.float()).t().repeat_interleave(32, dim=1)
    w_deq = w * torch.exp2(ew.float()).t().repeat_interleave(32, dim=1)
    ref = (a_deq.double() @ w_deq.double().t()).float() + bias
    exact = (ref.to(torch.bfloat16).float() + res).to(torch.bfloat16).float()         # bf16 result, then the residual added in bf16
    got = out.float().cpu()
    assert torch.equal(got, exact), float((got - exact).abs().max())


@pytest.mark.parametrize("M,N,K,act", [(4096, 768, 768, 0), (1025, 3072, 768, 1), (8200, 1024, 4096, 2)])
def test_mxfp8_persistent_linear_vs_fp32(dev, M, N, K, act):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    r = torch.randn(M, N, generator=g).to(torch.bfloat16)
    xq, xm = ops.quantize_mx_fp8(x.to(dev))
    wd = ops.mx_weight(w.to(dev))
    wq, wm = wd["q"], wd["mx"]
    out = ops.linear_mxfp8((xq, xm), wd, bias=b.to(dev), act=act, residual=r.to(dev)).float().cpu()
    fn = {0: lambda t: t, 1: torch.nn.functional.gelu, 2: lambda t: t * torch.sigmoid(1.702 * t)}[act]
    same = fn(_mx_deq(xq, xm, M, 128).cpu() @ _mx_deq(wq, wm, N, 64).cpu().t() + b.float()) + r.float()
    assert rel_err(out.numpy(), same.numpy()) < 4e-3
    full = fn(x.float() @ w.float().t() + b.float()) + r.float()
    e = rel_err(out.numpy(), full.numpy())
    print("mxfp8 linear M=%d N=%d K=%d: rel err vs unquantised fp32 %.4f" % (M, N, K, e))
    assert e < 0.05


@pytest.mark.parametrize("M,D,H", [(4099, 768, 3072), (8200, 1280, 5120), (700, 256, 512)])
def test_mxfp8_transformer_block_chain(dev, M, D, H):
    """The GEMM chain of a transformer block on the persistent MX kernel, no pass between the GEMMs:
       proj (+ residual; leaves bf16 x, its e4m3 + block-scale form and its rows' partial sums)
       -> LayerNorm folded into lin1 (+ GELU; only the e4m3 form of the hidden layer is written) -> lin2 (+ residual, same by-products).
    Every by-product against its definition, the chain against fp32."""
    g = torch.Generator().manual_seed(M)
    o = torch.randn(M, D, generator=g).to(torch.bfloat16)                       # attention output
    x0 = (torch.randn(M, D, generator=g) * 2 + 0.5).to(torch.bfloat16)          # residual stream (non-zero mean: the fold's cancellation)
    wp = (torch.randn(D, D, generator=g) / D ** 0.5).to(torch.bfloat16)
    w1 = (torch.randn(H, D, generator=g) / D ** 0.5).to(torch.bfloat16)
    w2 = (torch.randn(D, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    bp, b1, b2 = (torch.randn(n, generator=g).to(torch.bfloat16) for n in (D, H, D))
    gam = (1 + 0.2 * torch.randn(D, generator=g)).to(torch.bfloat16)
    bet = (0.2 * torch.randn(D, generator=g)).to(torch.bfloat16)
    eps = 1e-6
    x1 = ops.linear_mxfp8(ops.quantize_mx_fp8(o.to(dev)), ops.mx_weight(wp.to(dev)), bias=bp.to(dev), residual=x0.to(dev), mx_out=True, row_partials=True)
    # by-products of the producer: MX form and partial sums of exactly the bf16 values it stored
    q_ref, s_ref = _mx_reference(x1.x.cpu())
    xq, xm = x1.mx
    assert torch.equal(xm[:, ops.mx_scale_index(M, dev)].cpu(), s_ref) and torch.equal(xq.cpu(), q_ref)
    part = x1.partials.cpu()[:, :M]                                              # [D / 256, M, 2]
    tiles = x1.x.float().cpu().view(M, D // 256, 256)
    assert torch.allclose(part[..., 0].t(), tiles.sum(-1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(part[..., 1].t(), (tiles * tiles).sum(-1), rtol=1e-5, atol=1e-3)
    # LayerNorm folded into lin1, GELU, e4m3-only output
    fold = ops.fold_layernorm_mx(gam.to(dev), bet.to(dev), w1.to(dev), b1.to(dev))
    h = ops.linear_mxfp8(x1, fold, act=1, ln_eps=eps, mx_out=True, bf16_out=False)
    assert h.x is None
    hq, hm = h.mx
    xf = x1.x.float().cpu()
    mean, var = xf.mean(1, keepdim=True), xf.var(1, unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    xd = _mx_deq(xq, xm, M, 128).cpu()
    wgd = _mx_deq(fold["q"], fold["mx"], H, 64).cpu()
    h_same = torch.nn.functional.gelu(rstd * (xd @ wgd.t() - mean * fold["colsum"].cpu()[None]) + fold["bias_f32"].cpu()[None])
    hd = _mx_deq(hq, hm, M, 128).cpu()
    assert rel_err(hd.numpy(), h_same.numpy()) < 0.03                             # one e4m3 rounding of the result
    h_full = torch.nn.functional.gelu(torch.nn.functional.layer_norm(xf, (D,), gam.float(), bet.float(), eps) @ w1.float().t() + b1.float())
    e_h = rel_err(hd.numpy(), h_full.numpy())
    # lin2 back onto the residual stream
    x2 = ops.linear_mxfp8((hq, hm), ops.mx_weight(w2.to(dev)), bias=b2.to(dev), residual=x1.x, mx_out=True, row_partials=True)
    y_full = h_full @ w2.float().t() + b2.float() + xf
    e_y = rel_err(x2.x.float().cpu().numpy(), y_full.numpy())
    print("mxfp8 block chain M=%d D=%d H=%d: hidden layer rel err vs fp32 %.4f, block output %.4f" % (M, D, H, e_h, e_y))
    assert e_h < 0.06 and e_y < 0.03
    q2, s2 = _mx_reference(x2.x.cpu())
    assert torch.equal(x2.mx[1][:, ops.mx_scale_index(M, dev)].cpu(), s2) and torch.equal(x2.mx[0].cpu(), q2)


@pytest.mark.parametrize("name", ["tiny", "vit_h3"])
def test_sam_encoder_fp8_vs_reference_golden(dev, name):
    """The encoder with its qkv / proj / MLP GEMMs in fp8 against the reference's fp32 output: the measured cost of config C5's operand
    type next to the bf16 path's error on the same golden."""
    c = cases.SAM_ENCODERS[name]
    gold = cases.load("sam_encoder_" + name)
    enc = build_encoder(c, dev)
    x = cases.sam_encoder_input(c).to(dev, torch.bfloat16)
    with torch.no_grad():
        e16 = rel_err(cases.tap_embedding(enc(x).float().cpu()).numpy(), gold["out"])
        for blk in enc.blocks:
            blk.gemm_dtype = "fp8"
        e8 = rel_err(cases.tap_embedding(enc(x).float().cpu()).numpy(), gold["out"])
    print("encoder %s: rel err vs reference fp32: bf16 GEMMs %.4f, fp8 GEMMs %.4f" % (name, e16, e8))
    assert e8 < 0.07 and e8 < 8 * e16 + 0.01           # measured 0.055 (tiny) / 0.049 (vit_h3) against 0.0085 / 0.0079 with bf16 GEMMs


def test_masks_with_fp8_encoder_vs_oracle(dev):
    """What config C5's operand type costs at the OUTPUT of the path: tiny SAM encoder (fp8 qkv / proj / MLP GEMMs) -> CTP -> prompt
    encoder -> mask decoder -> postprocess against the fp32 oracle, next to the bf16 path on the same inputs.  The stated, measured
    mIoU delta of the fp8 path (white-noise embedding: every pixel is a boundary pixel, the worst case for thresholded agreement)."""
    from oracle import projectors as oproj
    from oracle import sam as osam
    from tests.test_gpu_modules import load_into, pixel_iou
    from walkgpt_amd.walkgpt import WalkGPTGrounding
    c = cases.SAM_ENCODERS["tiny"]
    g = c["img"] // c["patch"]
    model = WalkGPTGrounding(sam=dict(embed_dim=c["embed_dim"], depth=c["depth"], heads=c["heads"], global_idx=c["global_idx"], img=c["img"]),
                             llm_hidden=64, with_clip=False)
    w_enc, w_dec = cases.sam_encoder_weights(c), cases.decoder_weights(5)
    wm, wt = cases.projector_weights(dict(cases.PROJECTORS["h64"]))
    load_into(model.visual_model.image_encoder, w_enc, "image_encoder.", dev)
    load_into(model.visual_model.prompt_encoder, w_dec, "prompt_encoder.", dev, strict=False)
    load_into(model.visual_model.mask_decoder, w_dec, "mask_decoder.", dev)
    load_into(model.out_mm_projector, {"x." + k: v for k, v in wm.items()}, "x.", dev)
    load_into(model.text_hidden_fcs[0], {"x." + k: v for k, v in wt.items()}, "x.", dev)
    model.visual_model.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data = \
        w_dec["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"].to(dev)
    x = cases.sam_encoder_input(c)
    hidden = [torch.randn(2, 64, generator=torch.Generator().manual_seed(3)), torch.randn(3, 64, generator=torch.Generator().manual_seed(4))]
    resize, orig = [(512, 384), (400, 512)], [(200, 150), (75, 96)]
    hid = [h.to(dev, torch.bfloat16) for h in hidden]
    out16 = model(x.to(dev, torch.bfloat16), None, hid, resize, orig)
    m16 = [m.clone() for m in out16["pred_masks"]]
    model.set_gemm_dtype("fp8")
    out8 = model(x.to(dev, torch.bfloat16), None, hid, resize, orig)
    w_all = dict(w_enc)
    w_all.update(w_dec)
    with torch.no_grad():
        emb = osam.image_encoder(w_all, x, dict(patch=c["patch"], depth=c["depth"], heads=c["heads"], global_idx=c["global_idx"], window=c["window"]))
        dpe = osam.dense_pe(w_all, (g, g))
        i16, i8 = [], []
        for i in range(2):
            pe = oproj.ctp(wt, hidden[i].to(torch.bfloat16).float())
            sparse, dense = osam.prompt_encoder_text(w_all, pe.reshape(-1, 1, 256), (g, g))
            masks, _ = osam.mask_decoder(w_all, emb[i:i + 1], dpe, sparse, dense)
            ref = osam.postprocess_masks(masks, c["img"], resize[i], orig[i])[:, 0].numpy()
            i16.append(pixel_iou(m16[i].cpu().numpy(), ref))
            i8.append(pixel_iou(out8["pred_masks"][i].cpu().numpy(), ref))
    print("thresholded masks vs the fp32 oracle (pixel IoU per image): bf16 GEMMs %s, fp8 GEMMs %s; mean delta %.4f"
          % (["%.4f" % v for v in i16], ["%.4f" % v for v in i8], float(np.mean(i16) - np.mean(i8))))
    # measured 0.9888 / 0.9978 (fp8) against 0.9972 / 0.9993 (bf16): 5e-3 of mIoU on masks where EVERY pixel is a boundary pixel; on the
    # confident-mask case (test_gpu_modules.test_end_to_end_confident_masks_vs_reference) the same operand type stays within 3e-4
    assert min(i8) > 0.98 and np.mean(i16) - np.mean(i8) < 0.012


def test_clip_tower_fp8_vs_standin_golden(dev):
    """The CLIP tower with q|k|v / out_proj / fc1 / fc2 on fp8 operands (opt-in: set_gemm_dtype("fp8", clip=True); config C5 keeps the tower
    in bf16) against the stand-in's fp32 features, next to the bf16 path on the same golden."""
    from types import SimpleNamespace
    from tests.test_gpu_modules import load_into
    from walkgpt_amd.clip_encoder import CLIPVisionTower
    c = cases.CLIPS["tiny"]
    gold = cases.load("clip_tiny")
    cfg = dict(hidden_size=c["dim"], intermediate_size=4 * c["dim"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
               image_size=c["img"], patch_size=14, layer_norm_eps=1e-5)
    args = SimpleNamespace(mm_vision_select_layer=c["select_layer"], pad_train_clip_images=True, resize_vision_tower=True,
                           resize_vision_tower_size=c["img"])
    tower = CLIPVisionTower("synthetic", args, config=cfg)
    load_into(tower.vision_tower, cases.clip_weights(c), "", dev)
    x, key_mask = cases.clip_inputs(c)
    with torch.no_grad():
        sel16, _ = tower(x.to(dev, torch.bfloat16), attention_mask=key_mask.to(dev))
        for layer in tower.vision_tower.vision_model.encoder.layers:
            layer.gemm_dtype = "fp8"
        sel8, pre8 = tower(x.to(dev, torch.bfloat16), attention_mask=key_mask.to(dev))
    e16, e8 = rel_err(sel16.float().cpu().numpy(), gold["sel"]), rel_err(sel8.float().cpu().numpy(), gold["sel"])
    print("CLIP tower (tiny): selected features rel err vs fp32: bf16 GEMMs %.4f, fp8 GEMMs %.4f" % (e16, e8))
    assert e8 < 0.08 and torch.isfinite(pre8[0].float()).all()
