"""Thin tensor-level wrappers over the C-ABI.  torch is plumbing only here: it owns the HBM buffers and the
stream; every arithmetic step is a wg_* call.  All wrappers raise on non-GPU tensors -- there is no CPU path."""
import torch

from . import _lib

ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU = 0, 1, 2, 3
_BF16 = torch.bfloat16


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current HIP stream's handle.  (torch.cuda.current_stream() builds a Stream object through three Python layers, ~4 us a call and one call per
    launch: a third of a millisecond of a 590-launch training step; the raw accessor is the same handle in ~0.3 us.)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.WalkgptHipError("walkgpt_amd ops need GPU (HIP) tensors; got a %s tensor" % t.device)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _rows(t):
    """View a [..., D] tensor as rows: returns (rows, D, leading dimension)."""
    assert t.stride(-1) == 1, "innermost dimension must be contiguous"
    if t.dim() == 1:
        return 1, t.shape[0], t.shape[0]
    if t.dim() == 2:
        return t.shape[0], t.shape[1], t.stride(0)
    assert t.is_contiguous(), "tensors with more than two dimensions must be contiguous"
    return t.numel() // t.shape[-1], t.shape[-1], t.shape[-1]


import contextlib as _contextlib
import threading as _threading

_tls = _threading.local()  # per-thread measurement state (no module-level mutable switches: two models / threads never interact)


@_contextlib.contextmanager
def time_gemms():
    """Measurement only (bench.py): inside the block every GEMM launch of THIS thread is bracketed by a pair of HIP events on its
    launch stream.  Yields the list that collects (kernel id, M, N, K, start_event, end_event); 17 = the LayerNorm-folded instance."""
    records = []
    prev = getattr(_tls, "gemm_records", None)
    _tls.gemm_records = records
    try:
        yield records
    finally:
        _tls.gemm_records = prev


def _timed(kid, M, N, K):
    """Opens the bracket around one GEMM launch: inside time_gemms() records its start event and returns the pair, else None.
    _checked(ev, rc, what) closes it after the launch.  (Two plain calls, no closure: this is on every launch's path.)"""
    rec = getattr(_tls, "gemm_records", None)
    if rec is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    rec.append((kid, M, N, K, ev[0], ev[1]))
    ev[0].record()
    return ev


def _checked(ev, rc, what):
    if ev is not None:
        ev[1].record()
    if rc != 0:
        _lib.check(rc, what)


def gemm_tile_for(M, N, K, lda, ldw, ldc, ldr, tail_tiles=False):
    """Which kernel wg_gemm_bias_act_bf16 runs for this shape: 1 = 128x128 tiles, 2 = 256x256 tiles,
    3 = row-wave (asks the library's own selector, so host-side accounting and the library agree).
    tail_tiles: also consider the tail-absorbing 128x128 kernel (wg_gemm_pick_tile_ex in csrc/gemm.hip; single-stream callers)."""
    ok = K % 64 == 0 and N % 4 == 0 and N >= 16 and lda % 8 == 0 and ldw % 8 == 0 and ldc % 4 == 0 and ldr % 4 == 0
    if not ok:
        return 3
    return _lib.lib().wg_gemm_pick_tile_mnk(M, N, K, 1 if tail_tiles else 0)


GEMM_STAGED = 64  # flag bit of gemm_route's answer: the kernel runs the staged epilogue


def gemm_route(x, weight, bias=None, residual=None, out=None, tile=0, tail_tiles=False, res_row_mod=0, out_f32=False):
    """The kernel linear(x, weight, bias, residual=residual, out=out, tile=tile, tail_tiles=tail_tiles) launches for these tensors, by the
    launcher's own decision (wg_gemm_route_of: shape, leading dimensions, pointer alignment, the fallbacks), + GEMM_STAGED when that
    kernel runs the staged epilogue.  out None: a new contiguous tensor, fp32 with out_f32.  Launches nothing."""
    _need_gpu(x, weight, bias, residual, out)
    M, K, lda = _rows(x)
    N = weight.shape[0]
    ldc = N if out is None else _rows(out)[2]
    f32 = out_f32 if out is None else out.dtype == torch.float32
    ldr = _residual_ld(residual)
    if tile == 0:
        tile = gemm_tile_for(M, N, K, lda, weight.stride(0), ldc, ldr, tail_tiles)
    bits = 0
    for i, t in enumerate((x, weight, out, bias, residual)):
        bits |= (_ptr(t) & 15) << (4 * i)
    return _lib.lib().wg_gemm_route_of(M, N, K, lda, weight.stride(0), ldc, ldr, 0 if residual is None else 1, res_row_mod, 1 if f32 else 0,
                                       bits, tile)


class Rows:
    """Activation rows on their way from one GEMM to the next, with the by-products the producing kernel left beside them:
    x         bf16 [..., D]; None where only the fp8 form exists (the MLP hidden layer of the MX chain);
    partials  fp32 [D / 256, mpad, 2], the rows' {sum, sum of squares} per 256-column tile (mpad: rows padded to whole tiles), or None;
    mx        (e4m3 bytes [..., D], E8M0 block-scale planes [D / 32, mx_pitch(rows)]), or None.
    A Rows is a value: its x is not written after the Rows is made.  A torch in-place edit of x moves x._version, and fresh() then hands
    out neither by-product (the consumer runs its own pass); a write through x's raw pointer -- any wrapper's `out=` -- cannot be seen."""
    __slots__ = ("x", "partials", "mx", "_version")

    def __init__(self, x=None, partials=None, mx=None):
        self.x, self.partials, self.mx = x, partials, mx
        self._version = None if x is None else x._version

    def fresh(self):
        """(partials, mx) while x is as it was when they were made, else (None, None)."""
        if self.x is not None and self.x._version != self._version:
            return None, None
        return self.partials, self.mx


def _out(out, x, N, dtype=_BF16):
    """The result tensor [..., N] of a GEMM on rows x: the caller's `out`, else a new one."""
    return torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=dtype) if out is None else out


def _residual_ld(residual):
    """Leading dimension of a bf16 residual operand (0: none)."""
    if residual is None:
        return 0
    assert residual.dtype == _BF16
    return _rows(residual)[2]


def linear(x, weight, bias=None, act=ACT_NONE, residual=None, res_row_mod=0, out=None, out_f32=False, tile=0, tail_tiles=False,
           row_partials=False):
    """y = act(x @ weight.T + bias) (+ residual).  x [..., K] bf16, weight [N, K] bf16.
    row_partials: y feeds a LayerNorm that ln_linear folds into the next GEMM -- the result is a Rows; where the shape allows it the
    GEMM also leaves the per-row partial sums of y in it (wg_gemm_bias_act_stats_bf16) and ln_linear(rows, ...) reads them instead of
    running a statistics pass (partials None: the shape does not take that kernel)."""
    _need_gpu(x, weight, bias, residual, out)
    assert x.dtype == _BF16 and weight.dtype == _BF16
    M, K, lda = _rows(x)
    N, K2 = weight.shape
    assert K2 == K and weight.stride(1) == 1
    out = _out(out, x, N, torch.float32 if out_f32 else _BF16)
    Mo, No, ldc = _rows(out)
    assert Mo == M and No == N
    ldr = _residual_ld(residual)
    assert residual is None or residual.shape[-1] == N
    if bias is not None:
        assert bias.dtype == _BF16 and bias.numel() == N
    if (row_partials and not out_f32 and tile == 0 and not tail_tiles
            and _lib.lib().wg_gemm_row_partials_supported(M, N, K, lda, weight.stride(0), ldc)
            and (bias is None or bias.data_ptr() % 16 == 0) and (residual is None or (ldr % 8 == 0 and residual.data_ptr() % 16 == 0))):
        mpad = (M + 255) // 256 * 256
        part = torch.empty(N // 256, mpad, 2, device=x.device, dtype=torch.float32)
        ev = _timed(18, M, N, K)  # 18: the statistics-producing instance of kernel 16
        rc = _lib.lib().wg_gemm_bias_act_stats_bf16(x.data_ptr(), lda, weight.data_ptr(), weight.stride(0), _ptr(bias), _ptr(residual), ldr,
                                                    res_row_mod, out.data_ptr(), ldc, M, N, K, act, part.data_ptr(), mpad, _stream())
        _checked(ev, rc, "wg_gemm_bias_act_stats_bf16")
        return Rows(out, part)
    if tile == 0:
        tile = gemm_tile_for(M, N, K, lda, weight.stride(0), ldc, ldr, tail_tiles)
    ev = _timed(tile, M, N, K)
    rc = _lib.lib().wg_gemm_bias_act_bf16(x.data_ptr(), lda, weight.data_ptr(), weight.stride(0), _ptr(bias),
                                          _ptr(residual), ldr, res_row_mod, out.data_ptr(), ldc, M, N, K, act,
                                          1 if out.dtype == torch.float32 else 0, tile, _stream())
    _checked(ev, rc, "wg_gemm_bias_act_bf16")
    return Rows(out) if row_partials else out


def layernorm(x, gamma, beta, eps, act=ACT_NONE, out=None):
    _need_gpu(x, gamma, beta, out)
    assert x.dtype == _BF16 and gamma.dtype == _BF16 and beta.dtype == _BF16
    M, D, ldx = _rows(x)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=_BF16)
    _, _, ldy = _rows(out)
    rc = _lib.lib().wg_layernorm_rows(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), ldy, M, D,
                                      float(eps), act, _stream())
    _lib.check(rc, "wg_layernorm_rows")
    return out


def fold_layernorm(gamma, beta, weight, bias):
    """Operands of ln_linear: the LayerNorm's affine map folded into the linear layer that consumes it.
    y = LN(x) W^T + b = rstd (x Wg^T - mean s) + b'  with  Wg = bf16(W gamma), s = row sums of Wg (fp32, of the ROUNDED
    Wg, so the mean term cancels exactly what the MFMA accumulates), b' = b + W beta (fp32)."""
    wf = weight.float()
    wg = (wf * gamma.float()[None, :]).to(_BF16).contiguous()
    b = wf @ beta.float()
    if bias is not None:
        b = b + bias.float()
    return {"wg": wg, "colsum": wg.float().sum(1).contiguous(), "bias_f32": b.contiguous(),
            "gamma": gamma, "beta": beta, "weight": weight, "bias": bias}


def row_stats(x, eps):
    """(mean, 1/sqrt(var + eps)) per row of x [..., D] bf16 -> fp32 [rows rounded up to even, 2]."""
    _need_gpu(x)
    M, D, ldx = _rows(x)
    st = torch.empty((M + 1) // 2 * 2, 2, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_row_stats_bf16(x.data_ptr(), ldx, st.data_ptr(), M, D, float(eps), _stream()), "wg_row_stats_bf16")
    return st


def ln_linear(x, fold, eps, act=ACT_NONE, tail_tiles=False):
    """act(LayerNorm(x) @ W.T + b) with `fold` from fold_layernorm; x a tensor or a Rows.  Shapes the persistent 256x256 GEMM takes run
    as one GEMM on the raw rows (the normalised rows never reach HBM), on the Rows' partial sums where it has fresh ones and behind a
    row-statistics pass otherwise; the rest as LayerNorm + GEMM."""
    part = None
    if isinstance(x, Rows):
        part, x = x.fresh()[0], x.x
    _need_gpu(x)
    assert x.dtype == _BF16
    M, K, lda = _rows(x)
    N = fold["wg"].shape[0]
    L = _lib.lib()
    if not L.wg_gemm_ln_supported(M, N, K, lda, K, N):
        return linear(layernorm(x, fold["gamma"], fold["beta"], eps), fold["weight"], fold["bias"], act=act, tail_tiles=tail_tiles)
    out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=_BF16)
    if part is not None:
        # the GEMM that wrote x left its rows' partial sums (linear(..., row_partials=True)): no statistics pass
        assert part.shape[0] * 256 == K and part.shape[1] >= M
        ev = _timed(17, M, N, K)
        rc = L.wg_gemm_lnp_bias_act_bf16(x.data_ptr(), lda, fold["wg"].data_ptr(), K, fold["bias_f32"].data_ptr(), fold["colsum"].data_ptr(),
                                         part.data_ptr(), part.shape[0], part.shape[1], float(eps), out.data_ptr(), N, M, N, K, act, _stream())
        _checked(ev, rc, "wg_gemm_lnp_bias_act_bf16")
        return out
    st = row_stats(x, eps)
    ev = _timed(17, M, N, K)  # 17: the LayerNorm-folded instance of kernel 16
    rc = L.wg_gemm_ln_bias_act_bf16(x.data_ptr(), lda, fold["wg"].data_ptr(), K, fold["bias_f32"].data_ptr(),
                                    fold["colsum"].data_ptr(), st.data_ptr(), out.data_ptr(), N, M, N, K, act, _stream())
    _checked(ev, rc, "wg_gemm_ln_bias_act_bf16")
    return out


def layernorm_linear(x, gamma, beta, eps, weight, bias=None, act=ACT_NONE, out_f32=False, weight_tiled=None):
    """act(LayerNorm(x) @ weight.T + bias) (gamma None: no LayerNorm) for a handful of rows (M <= 128: the [SEG] hidden states into
    text_hidden_fcs) in one launch (wg_gemm_skinny_ln_bias_act_bf16); other shapes run LayerNorm and the GEMM as two kernels.
    weight_tiled: tile_weight(weight), read instead of `weight` by the one-launch form."""
    _need_gpu(x, gamma, beta, weight, bias, weight_tiled)
    assert x.dtype == _BF16 and weight.dtype == _BF16
    M, K, lda = _rows(x)
    N = weight.shape[0]
    L = _lib.lib()
    if not L.wg_gemm_skinny_ln_supported(M, N, K, lda, weight.stride(0), N):
        return linear(x if gamma is None else layernorm(x, gamma, beta, eps), weight, bias, act=act, out_f32=out_f32)
    assert weight.shape[1] == K and weight.stride(1) == 1
    assert gamma is None or (gamma.dtype == _BF16 and beta.dtype == _BF16 and gamma.numel() == K and beta.numel() == K)
    assert weight_tiled is None or _tiled_ok(weight_tiled, N, K)
    out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32 if out_f32 else _BF16)
    ev = _timed(5, M, N, K)
    w = weight if weight_tiled is None else weight_tiled
    rc = L.wg_gemm_skinny_ln_bias_act_bf16(x.data_ptr(), lda, _ptr(gamma), _ptr(beta), float(eps), w.data_ptr(), weight.stride(0),
                                           0 if weight_tiled is None else 1, _ptr(bias), out.data_ptr(), N, M, N, K, act,
                                           1 if out_f32 else 0, _stream())
    _checked(ev, rc, "wg_gemm_skinny_ln_bias_act_bf16")
    return out


def _rows_per_batch(t):
    """[B, L, D] (contiguous rows, possibly a column slice of a wider buffer) -> (B, L, ld, rows per batch)."""
    assert t.dim() == 3 and t.stride(2) == 1
    B, L, _ = t.shape
    ld = t.stride(1)
    assert t.stride(0) % ld == 0 or B == 1
    return B, L, ld, (t.stride(0) // ld if B > 1 else L)


def _mha_takes_small(hd, Lq, Lk, has_key_bias, small):
    """mha()'s choice between wg_mha_small_bf16 (one wave per query) and wg_mha_bf16 (the tiled MFMA kernels)."""
    if small is None:
        small = hd < 32 or Lq <= 32 or Lk <= 32
    if small and not has_key_bias and Lq <= 32 and Lk >= 256 and hd in (16, 32, 64, 128):
        small = False  # few queries, many keys: one MFMA wave per (batch, head) reads K/V once for all queries
    return small


ROUTE_TILED, ROUTE_WINDOW, ROUTE_WINDOW_UNIT, ROUTE_PIPE, ROUTE_SMALL = 1, 2, 3, 4, 5


def route_code(family, hd, S=0, waves=1, key_bias=0):
    """The route codes of wg_mha_route / wg_sam_attn_route (include/walkgpt_hip.h); family ROUTE_SMALL (wg_mha_small_bf16, attn_small.hip:
    one wave per query, or one lane per query where few keys meet many queries) exists at this level only."""
    return family * 10000000 + hd * 10000 + S * 100 + waves * 10 + int(key_bias)


def mha_route(hd, Lq, Lk, has_key_bias=False, small=None):
    """Which kernel mha() would run for these shapes (under the current wg_attn_pipe_mode), as a route code; negative: none is compiled.
    Host arithmetic, needs no GPU."""
    if _mha_takes_small(hd, Lq, Lk, has_key_bias, small):
        return route_code(ROUTE_SMALL, hd) if hd in (16, 32, 64, 128) and not has_key_bias else -2
    return _lib.lib().wg_mha_route(hd, Lq, Lk, 1 if has_key_bias else 0)


def sam_attention_route(B, grid, window, heads, hd):
    """Which kernel sam_attention() would run (bf16 output), as a route code; negative: none is compiled."""
    return _lib.lib().wg_sam_attn_route(B, grid, window, heads, hd)


def mha(q, k, v, heads, scale, key_bias=None, out=None, small=None):
    """softmax(scale * q k^T + key_bias) v per head.  q [B,Lq,D], k/v [B,Lk,D] (bf16, may be column slices of a
    packed buffer); key_bias [B,Lk] fp32 additive or None.  `small` forces / forbids the one-wave-per-query kernel."""
    _need_gpu(q, k, v, key_bias, out)
    B, Lq, ldq, qbs = _rows_per_batch(q)
    _, Lk, ldk, kbs = _rows_per_batch(k)
    _, _, ldv, vbs = _rows_per_batch(v)
    assert kbs == vbs
    D = q.shape[2]
    hd = D // heads
    if out is None:
        out = torch.empty(B, Lq, D, device=q.device, dtype=_BF16)
    _, _, ldo, obs = _rows_per_batch(out)
    if _mha_takes_small(hd, Lq, Lk, key_bias is not None, small):
        assert key_bias is None
        rc = _lib.lib().wg_mha_small_bf16(q.data_ptr(), ldq, qbs, k.data_ptr(), ldk, v.data_ptr(), ldv, kbs,
                                          out.data_ptr(), ldo, obs, B, heads, hd, Lq, Lk, float(scale), _stream())
        _lib.check(rc, "wg_mha_small_bf16")
    else:
        if key_bias is not None:
            assert key_bias.dtype == torch.float32 and key_bias.is_contiguous() and key_bias.shape == (B, Lk)
        rc = _lib.lib().wg_mha_bf16(q.data_ptr(), ldq, qbs, k.data_ptr(), ldk, v.data_ptr(), ldv, kbs, out.data_ptr(),
                                    ldo, obs, _ptr(key_bias), B, heads, hd, Lq, Lk, float(scale), _stream())
        _lib.check(rc, "wg_mha_bf16")
    return out


def sam_attention(qkv, qkv_bias, rel_pos_h, rel_pos_w, B, grid, window, heads, out=None, mx_out=False):
    """SAM ViT attention over packed qkv rows [B*grid*grid, 3D]; window == grid means global attention.
    mx_out: the fp8 chain's form, a Rows -- where the kernels carry it (head_dim 64; window 14 or the 64 x 64 global grid) with mx alone:
    the (e4m3 bytes, E8M0 block scales) quantize_mx_fp8 would make of the bf16 output, written by the attention kernel itself; elsewhere
    with x alone, the bf16 tensor as usual (the caller quantises)."""
    _need_gpu(qkv, qkv_bias, rel_pos_h, rel_pos_w, out)
    D = qkv.shape[-1] // 3
    hd = D // heads
    assert qkv.is_contiguous() and qkv.shape[0] == B * grid * grid and qkv.dtype == _BF16
    assert rel_pos_h.shape == (2 * window - 1, hd) and rel_pos_h.is_contiguous() and rel_pos_w.is_contiguous()
    if mx_out and out is None and _lib.lib().wg_sam_attn_mx_supported(B, grid, window, heads, hd):
        M = B * grid * grid
        q = torch.empty(M, D, device=qkv.device, dtype=torch.uint8)
        mx = torch.empty(D // 32, mx_pitch(M), device=qkv.device, dtype=torch.uint8)
        rc = _lib.lib().wg_sam_attn_relpos_mx_bf16(qkv.data_ptr(), qkv_bias.data_ptr(), rel_pos_h.data_ptr(), rel_pos_w.data_ptr(), q.data_ptr(), mx.data_ptr(),
                                                   mx.shape[1], B, grid, window, heads, hd, float(hd) ** -0.5, _stream())
        _lib.check(rc, "wg_sam_attn_relpos_mx_bf16")
        return Rows(mx=(q, mx))
    if out is None:
        out = torch.empty(B * grid * grid, D, device=qkv.device, dtype=_BF16)
    rc = _lib.lib().wg_sam_attn_relpos_bf16(qkv.data_ptr(), qkv_bias.data_ptr(), rel_pos_h.data_ptr(),
                                            rel_pos_w.data_ptr(), out.data_ptr(), B, grid, window, heads, hd,
                                            float(hd) ** -0.5, _stream())
    _lib.check(rc, "wg_sam_attn_relpos_bf16")
    return Rows(out) if mx_out else out


def patchify(images, patch, kpad=None):
    """NCHW bf16 images -> [B*gh*gw, kpad] rows in conv-weight column order, zero padded to kpad columns."""
    _need_gpu(images)
    assert images.dtype == _BF16 and images.is_contiguous()
    B, C, H, W = images.shape
    K = C * patch * patch
    kpad = kpad or ((K + 63) // 64) * 64
    rows = torch.empty(B * (H // patch) * (W // patch), kpad, device=images.device, dtype=_BF16)
    rc = _lib.lib().wg_patchify_bf16(images.data_ptr(), rows.data_ptr(), B, C, H, W, patch, kpad, _stream())
    _lib.check(rc, "wg_patchify_bf16")
    return rows


def im2row3x3(x, B, H, W):
    _need_gpu(x)
    C = x.shape[-1]
    assert x.is_contiguous() and x.numel() == B * H * W * C
    rows = torch.empty(B * H * W, 9 * C, device=x.device, dtype=_BF16)
    rc = _lib.lib().wg_im2row3x3_bf16(x.data_ptr(), rows.data_ptr(), B, H, W, C, _stream())
    _lib.check(rc, "wg_im2row3x3_bf16")
    return rows


def add_rows(a, b, out=None):
    """a [..., C] + b [rb, C] broadcast by row index modulo rb."""
    _need_gpu(a, b, out)
    rows, cols, lda = _rows(a)
    rb, cb, ldb = _rows(b)
    assert cb == cols
    if out is None:
        out = torch.empty(a.shape, device=a.device, dtype=_BF16)
    _, _, ldo = _rows(out)
    rc = _lib.lib().wg_add_rows_bf16(a.data_ptr(), lda, b.data_ptr(), ldb, rb, out.data_ptr(), ldo, rows, cols, _stream())
    _lib.check(rc, "wg_add_rows_bf16")
    return out


def tokens_to_nchw(x, B, HW, C):
    _need_gpu(x)
    assert x.is_contiguous()
    y = torch.empty(B, C, HW, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_tokens_to_nchw_bf16(x.data_ptr(), y.data_ptr(), B, HW, C, _stream()), "wg_tokens_to_nchw_bf16")
    return y


def nchw_to_tokens(x):
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == _BF16
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty(B, HW, C, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_nchw_to_tokens_bf16(x.data_ptr(), y.data_ptr(), B, HW, C, _stream()), "wg_nchw_to_tokens_bf16")
    return y


def dense_pe_tokens(gaussian, h, w):
    """[h*w, 2F] fp32 positional encoding rows from the [2, F] fp32 gaussian matrix."""
    _need_gpu(gaussian)
    g = gaussian.float().contiguous()
    F_ = g.shape[1]
    pe = torch.empty(h * w, 2 * F_, device=g.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_dense_pe_f32(g.data_ptr(), pe.data_ptr(), h, w, F_, _stream()), "wg_dense_pe_f32")
    return pe


def cast_bf16(x):
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty(x.shape, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_cast_f32_to_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "wg_cast_f32_to_bf16")
    return y


def prompt_sparse(coords, labels, pad, boxes, text, gaussian, embed_table, image_size):
    """Sparse prompt rows (wg_prompt_sparse_f32): coords [B,N,2] fp32 + labels [B,N] int32 (or None), boxes [B,4] fp32 (or None), text [B,T,C]
    bf16 / fp32 (or None); gaussian [2, C/2] fp32, embed_table [5, C] fp32 -> fp32 [B, N + pad + 2 * has_box + T, C]."""
    _need_gpu(coords, labels, boxes, text, gaussian, embed_table)
    C = embed_table.shape[1]
    assert gaussian.dtype == torch.float32 and gaussian.is_contiguous() and tuple(gaussian.shape) == (2, C // 2)
    assert embed_table.dtype == torch.float32 and embed_table.is_contiguous() and embed_table.shape[0] == 5
    B, N = (coords.shape[0], coords.shape[1]) if coords is not None else (boxes.shape[0], 0)
    if coords is not None:
        assert coords.dtype == torch.float32 and coords.is_contiguous() and coords.shape == (B, N, 2)
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape == (B, N)
    if boxes is not None:
        assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape == (B, 4)
    T = 0
    if text is not None:
        assert text.dtype in (_BF16, torch.float32) and text.is_contiguous() and text.dim() == 3 and text.shape[0] == B and text.shape[2] == C
        T = text.shape[1]
    R = (N + int(pad) if coords is not None else 0) + (2 if boxes is not None else 0) + T
    out = torch.empty(B, R, C, device=embed_table.device, dtype=torch.float32)
    rc = _lib.lib().wg_prompt_sparse_f32(_ptr(coords), _ptr(labels), B, N, int(pad), _ptr(boxes), _ptr(text), T, 1 if text is not None and
                                         text.dtype == _BF16 else 0, gaussian.data_ptr(), embed_table.data_ptr(), C, int(image_size[0]),
                                         int(image_size[1]), out.data_ptr(), _stream())
    _lib.check(rc, "wg_prompt_sparse_f32")
    return out


def mask_embed(masks, params, eps1, eps2, mask_in_chans=16, embed_dim=256):
    """PromptEncoder.mask_downscaling (wg_mask_embed_bf16): masks fp32 [B,1,4h,4w] -> bf16 channel-last rows [B, h*w, embed_dim];
    params: the fp32 blob the C-ABI documents."""
    _need_gpu(masks, params)
    assert masks.dtype == torch.float32 and masks.is_contiguous() and masks.dim() == 4 and masks.shape[1] == 1
    assert params.dtype == torch.float32 and params.is_contiguous()
    B, _, H, W = masks.shape
    if H % 4 or W % 4:
        raise ValueError("mask inputs must be 4h x 4w (got %d x %d)" % (H, W))
    h, w = H // 4, W // 4
    out = torch.empty(B, h * w, embed_dim, device=masks.device, dtype=_BF16)
    rc = _lib.lib().wg_mask_embed_bf16(masks.data_ptr(), params.data_ptr(), float(eps1), float(eps2), out.data_ptr(), B, h, w, mask_in_chans,
                                       embed_dim, _stream())
    _lib.check(rc, "wg_mask_embed_bf16")
    return out


def normalize_pad(x, mean, std, size, out=None):
    """Sam.preprocess (wg_normalize_pad_bf16): x [B,3,H,W] uint8 or fp32, mean / std fp32 [3] -> bf16 [B,3,size,size]."""
    _need_gpu(x, mean, std, out)
    assert x.dtype in (torch.uint8, torch.float32) and x.is_contiguous() and x.dim() == 4 and x.shape[1] == 3
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and mean.numel() == 3 and std.numel() == 3
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty(B, 3, size, size, device=x.device, dtype=_BF16)
    assert out.dtype == _BF16 and out.is_contiguous() and tuple(out.shape) == (B, 3, size, size)
    rc = _lib.lib().wg_normalize_pad_bf16(x.data_ptr(), 1 if x.dtype == torch.uint8 else 0, mean.data_ptr(), std.data_ptr(), out.data_ptr(), B, H,
                                          W, size, _stream())
    _lib.check(rc, "wg_normalize_pad_bf16")
    return out


def hyper_mask_dot(up, hyper, T, h, w, first_mask, num_masks):
    """up: pixel-shuffled upscaled embedding rows [T*h*w*4, 4*32]; hyper [T, nmask, 32] -> fp32 [T, num_masks, 4h, 4w]."""
    _need_gpu(up, hyper)
    assert up.is_contiguous() and hyper.is_contiguous() and up.shape == (T * h * w * 4, 128)
    masks = torch.empty(T, num_masks, 4 * h, 4 * w, device=up.device, dtype=torch.float32)
    rc = _lib.lib().wg_hyper_mask_dot(up.data_ptr(), hyper.data_ptr(), masks.data_ptr(), T, h, w, 32, hyper.shape[1],
                                      first_mask, num_masks, _stream())
    _lib.check(rc, "wg_hyper_mask_dot")
    return masks


def quantize_rows_fp8(x, ln=None, eps=0.0):
    """Per-row e4m3 quantisation of x [..., K] bf16 (of LayerNorm(x) when ln = (gamma, beta)) -> (q uint8 [..., K], scale fp32 [rows])."""
    _need_gpu(x)
    assert x.dtype == _BF16
    M, K, ldx = _rows(x)
    q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    scale = torch.empty(M, device=x.device, dtype=torch.float32)
    L = _lib.lib()
    if ln is None:
        rc = L.wg_quantize_rows_fp8(x.data_ptr(), ldx, q.data_ptr(), K, scale.data_ptr(), M, K, _stream())
    else:
        g, b = ln
        _need_gpu(g, b)
        rc = L.wg_layernorm_quantize_fp8(x.data_ptr(), ldx, g.data_ptr(), b.data_ptr(), float(eps), q.data_ptr(), K, scale.data_ptr(), M, K, _stream())
    _lib.check(rc, "wg_quantize_rows_fp8")
    return q, scale


def quantize_weight_fp8(weight):
    """nn.Linear weight [N, K] bf16 -> (e4m3 bytes [N, K], per-output-channel scale fp32 [N]); once per weight set."""
    return quantize_rows_fp8(weight.contiguous())


def mx_pitch(M):
    """Row pitch (bytes) of an MX block-scale plane for M rows: whole 256-row tiles."""
    return (M + 255) // 256 * 256


def mx_scale_index(M, device=None, group=128):
    """Position of row m inside a block-scale plane (include/walkgpt_hip.h: wg_gemm_mxfp8): rows of a `group`-row group are
    permuted to (r % 16) * (group / 16) + r // 16 (128: activations, 64: weights).  For tests and tools; the kernels never materialise it."""
    m = torch.arange(M, device=device)
    r = m % group
    return (m - r) + (r % 16) * (group // 16) + r // 16


def quantize_mx_fp8(x, group=128, row_partials=False):
    """x [..., K] bf16 -> (e4m3 bytes uint8 [..., K], E8M0 block scales uint8 [K / 32, mx_pitch(rows)]): OCP-MX, one power-of-two scale per
    (row, 32 columns).  group=128: an activation operand of linear_mxfp8; group=64: its weight operand (once per weight).
    row_partials (K % 256 == 0): the same pass also makes x's row partial sums, as a GEMM epilogue would have, and returns them third."""
    _need_gpu(x)
    assert x.dtype == _BF16
    M, K, ldx = _rows(x)
    q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    mx = torch.empty(K // 32, mx_pitch(M), device=x.device, dtype=torch.uint8)
    part = torch.empty(K // 256, mx_pitch(M), 2, device=x.device, dtype=torch.float32) if row_partials else None
    rc = _lib.lib().wg_quantize_mx_fp8(x.data_ptr(), ldx, q.data_ptr(), K, mx.data_ptr(), mx.shape[1], group, M, K, _ptr(part),
                                       part.shape[1] if row_partials else 0, _stream())
    _lib.check(rc, "wg_quantize_mx_fp8")
    return (q, mx, part) if row_partials else (q, mx)


def mx_dequantize(q, mx, group=128):
    """(e4m3 bytes [rows, K], block scales [K / 32, pitch]) -> fp32 values (host-side helper: weight folds, tests)."""
    rows, K = q.shape
    e = mx[:, mx_scale_index(rows, mx.device, group)].float() - 127.0          # [K/32, rows]
    return (q.view(torch.float8_e4m3fn).float().view(rows, K // 32, 32) * torch.exp2(e).t()[..., None]).view(rows, K)


def mx_weight(weight):
    """nn.Linear weight [N, K] bf16 -> {"q", "mx"}: the W operand of linear_mxfp8 (once per weight set)."""
    q, mx = quantize_mx_fp8(weight.contiguous(), group=64)
    return {"q": q, "mx": mx}


def fold_layernorm_mx(gamma, beta, weight, bias):
    """fold_layernorm for the fp8 path: Wg = W gamma quantised to e4m3 with MX block scales, s = row sums of the DEQUANTISED Wg (so the
    mean term cancels exactly what the block-scaled MFMA accumulates), b' = b + W beta (fp32, from the unquantised weight)."""
    wf = weight.float()
    q, mx = quantize_mx_fp8((wf * gamma.float()[None, :]).to(_BF16).contiguous(), group=64)
    b = wf @ beta.float()
    if bias is not None:
        b = b + bias.float()
    return {"q": q, "mx": mx, "colsum": mx_dequantize(q, mx, 64).sum(1).contiguous(), "bias_f32": b.contiguous()}


def mx_chain_ok(D, hidden):
    """Can a transformer block of width D / MLP width `hidden` run its four linears as one MX chain on the persistent fp8 GEMM?  (LayerNorm
    fold: the row statistics arrive as D / 256 partial planes, at most 5; fp8 copies need whole 32-column blocks.)"""
    return D % 256 == 0 and D <= 1280 and hidden % 32 == 0 and hidden % 128 == 0


def mx_rows(x):
    """bf16 activation rows [.., D] (D % 256 == 0; a tensor or a Rows) -> a Rows with what an MX-chain consumer (linear_mxfp8(ln_eps=...))
    expects: x, its e4m3 + block-scale form and its rows' partial sums.  Inside the chain the producing GEMM's epilogue leaves both; at
    the chain's entry one quantisation pass makes what is missing."""
    r = x if isinstance(x, Rows) else Rows(x)
    part, mx = r.fresh()
    if mx is None or part is None:
        got = quantize_mx_fp8(r.x, row_partials=part is None)
        r = Rows(r.x, got[2] if part is None else part, got[:2])
    return r


def linear_mxfp8(x, w, bias=None, act=ACT_NONE, residual=None, res_row_mod=0, out=None, ln_eps=None, mx_out=False, bf16_out=True,
                 row_partials=False):
    """act(dequant(x) @ dequant(w).T + bias) (+ residual) on the persistent fp8 GEMM with MX block scales on both operands.
    x: a Rows whose mx is read (from an earlier call's mx_out, mx_rows or sam_attention); a bare (xq uint8 [..., K], x_mx) pair from
       quantize_mx_fp8 stands for Rows(mx=pair).  With ln_eps set its partials are read too: LayerNorm(x) is folded in and
       w = fold_layernorm_mx(...);
    w: mx_weight(...) / fold_layernorm_mx(...).
    mx_out: the result also leaves as e4m3 + block scales (with bf16_out=False ONLY so); row_partials: with its rows' {sum, sum of
    squares} partials (N % 256 == 0).  With either the result is a Rows (x None with bf16_out=False), else the bf16 tensor."""
    ln, xmx = (x if isinstance(x, Rows) else Rows(mx=x)).fresh()
    if ln_eps is None:
        ln = None
    elif ln is None:
        raise ValueError("linear_mxfp8(ln_eps=...): x has no fresh partials (ops.mx_rows makes them)")
    if xmx is None:
        raise ValueError("linear_mxfp8: x has no fresh mx (ops.mx_rows / ops.quantize_mx_fp8 make one)")
    xq, x_mx = xmx
    wq, w_mx = w["q"], w["mx"]
    _need_gpu(xq, x_mx, wq, w_mx, bias, residual, out)
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and xq.is_contiguous() and wq.is_contiguous()
    assert x_mx.dtype == torch.uint8 and w_mx.dtype == torch.uint8 and x_mx.is_contiguous() and w_mx.is_contiguous()
    K = xq.shape[-1]
    M = xq.numel() // K
    N = wq.shape[0]
    assert wq.shape[1] == K and x_mx.shape[0] == K // 32 and w_mx.shape[0] == K // 32
    dev = xq.device
    assert bf16_out or mx_out
    assert ln is None or (ln.shape[0] * 256 == K and ln.shape[1] >= M)
    if out is None and bf16_out:
        out = torch.empty(xq.shape[:-1] + (N,), device=dev, dtype=_BF16)
    ldc = _rows(out)[2] if out is not None else 0
    ldr = _residual_ld(residual)
    cq = cmx = part = None
    if mx_out:
        cq = torch.empty(xq.shape[:-1] + (N,), device=dev, dtype=torch.uint8)
        cmx = torch.empty(N // 32, mx_pitch(M), device=dev, dtype=torch.uint8)
    if row_partials:
        assert N % 256 == 0 and ln is None
        part = torch.empty(N // 256, mx_pitch(M), 2, device=dev, dtype=torch.float32)
    ev = _timed(22 if ln is not None else (23 if row_partials else 21), M, N, K)   # (ids: bench.py KERNEL_NAMES)
    rc = _lib.lib().wg_gemm_mxfp8(xq.data_ptr(), K, x_mx.data_ptr(), x_mx.shape[1], wq.data_ptr(), K, w_mx.data_ptr(), w_mx.shape[1],
                                  None if ln is not None else _ptr(bias),
                                  w["colsum"].data_ptr() if ln is not None else None, w["bias_f32"].data_ptr() if ln is not None else None,
                                  ln.data_ptr() if ln is not None else None, ln.shape[0] if ln is not None else 0,
                                  ln.shape[1] if ln is not None else 0, float(ln_eps) if ln is not None else 0.0,
                                  _ptr(residual), ldr, res_row_mod, _ptr(out), ldc, _ptr(cq), N, _ptr(cmx), cmx.shape[1] if mx_out else 0,
                                  _ptr(part), part.shape[1] if row_partials else 0, M, N, K, act, _stream())
    _checked(ev, rc, "wg_gemm_mxfp8")
    if mx_out or row_partials:
        return Rows(out, part, (cq, cmx) if mx_out else None)
    return out


def linear_fp8(xq, x_scale, wq, w_scale, bias=None, act=ACT_NONE, residual=None, res_row_mod=0, out=None):
    """act(dequant(xq) @ dequant(wq).T + bias) (+ residual) -> bf16.  xq [..., K] uint8 (e4m3) with per-row scales, wq [N, K] with
    per-output-channel scales (quantize_rows_fp8 / quantize_weight_fp8).  The form for widths the MX chain (linear_mxfp8) does not take."""
    _need_gpu(xq, x_scale, wq, w_scale, bias, residual, out)
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and xq.is_contiguous() and wq.is_contiguous()
    K = xq.shape[-1]
    M = xq.numel() // K
    N = wq.shape[0]
    assert wq.shape[1] == K and x_scale.numel() == M and w_scale.numel() == N
    out = _out(out, xq, N)
    _, _, ldc = _rows(out)
    ldr = _residual_ld(residual)
    ev = _timed(20, M, N, K)
    rc = _lib.lib().wg_gemm_fp8_bias_act(xq.data_ptr(), K, x_scale.data_ptr(), wq.data_ptr(), K, w_scale.data_ptr(), _ptr(bias),
                                         _ptr(residual), ldr, res_row_mod, out.data_ptr(), ldc, M, N, K, act, _stream())
    _checked(ev, rc, "wg_gemm_fp8_bias_act")
    return out


def tile_weight(w, k_slices=1):
    """Weight matrix [N, K] bf16 -> fragment order [k_slices, ceil(N / 16), K / (32 k_slices), 64, 8] for the token-side decoder kernels
    (wg_tile_weight_bf16; squeezed to 4-D when k_slices == 1).  k_slices > 1 tiles each K-slice on its own (mlp.lin2 of the two-way block)."""
    _need_gpu(w)
    assert w.dtype == _BF16 and w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    assert K % (32 * k_slices) == 0
    ks = K // k_slices
    out = torch.empty(k_slices, (N + 15) // 16, ks // 32, 64, 8, device=w.device, dtype=_BF16)
    for s in range(k_slices):
        rc = _lib.lib().wg_tile_weight_bf16(w.data_ptr() + 2 * s * ks, w.stride(0), N, ks, out[s].data_ptr(), _stream())
        _lib.check(rc, "wg_tile_weight_bf16")
    return out[0] if k_slices == 1 else out


def _tiled_ok(t, N, K, k_slices=1):
    shape = ((N + 15) // 16, K // (32 * k_slices), 64, 8)
    return t.dtype == _BF16 and t.is_contiguous() and tuple(t.shape) == ((k_slices,) + shape if k_slices > 1 else shape)


TOK_SUM_MLP, TOK_SELF, TOK_Q_T2I, TOK_COMBINE, TOK_INIT = 1, 2, 4, 8, 16
_TOK_PART = 6 * 18          # floats of one attention partial (csrc/decoder.hip)


def _f32_tokens(t, P, last):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (P, 6, last), (t.dtype, tuple(t.shape))


def dec_tokens(stages, skip_pe, queries, query_pe, weights, q_t2i=None, attn_partials=None, mlp_partials=None, k_i2t=None, v_i2t=None,
               eps=1e-5, init_tokens=None, init_prompt=None, prompt_tail=None):
    """Per-prompt stages of the token side of SAM's two-way transformer (csrc/decoder.hip: wg_dec_tokens_f32; stage bits TOK_*).
    queries / query_pe [P, 6, 256] fp32 (queries updated in place); weights: the 24-slot table the C-ABI documents (bf16 tensors or
    None for the slots of stages that do not run; the weight matrices in fragment order, ops.tile_weight).  TOK_INIT: queries and query_pe are OUTPUTS, both set to
    cat(init_tokens [5, 256] fp32, init_prompt [P, 256] bf16) before the other stages run; with prompt_tail = (gamma, beta, text_type, log_temp
    bf16 tensors, eps) init_prompt holds the text projector's rows BEFORE its tail and the launch applies the tail (wg_dec_tokens_ctp_f32: same
    bits as ops.ctp_tail followed by the plain launch)."""
    import ctypes
    _need_gpu(queries, query_pe, q_t2i, attn_partials, mlp_partials, k_i2t, v_i2t, init_tokens, init_prompt, *weights)
    P = queries.shape[0]
    _f32_tokens(queries, P, 256)
    _f32_tokens(query_pe, P, 256)
    assert len(weights) == 24 and all(w is None or (w.dtype == _BF16 and w.is_contiguous()) for w in weights)
    n_splits = 0
    if stages & TOK_INIT:
        assert init_tokens.dtype == torch.float32 and init_tokens.is_contiguous() and init_tokens.shape == (5, 256)
        assert init_prompt.dtype == _BF16 and init_prompt.is_contiguous() and init_prompt.numel() == P * 256
    if stages & TOK_Q_T2I:
        _f32_tokens(q_t2i, P, 128)
    if stages & TOK_COMBINE:
        assert attn_partials.dtype == torch.float32 and attn_partials.is_contiguous() and attn_partials.dim() == 4
        assert attn_partials.shape[0] == P and attn_partials.shape[1] == 8 and attn_partials.shape[3] == _TOK_PART
        n_splits = attn_partials.shape[2]
    if stages & TOK_SUM_MLP:
        assert mlp_partials.dtype == torch.float32 and mlp_partials.is_contiguous() and mlp_partials.shape == (P, dec_mlp_slices(), 6, 256)
        for t in (k_i2t, v_i2t):
            assert t.dtype == _BF16 and t.is_contiguous() and t.shape == (P, 6, 128)
    table = (ctypes.c_void_p * 24)(*[None if w is None else w.data_ptr() for w in weights])
    if prompt_tail is not None:
        assert stages & TOK_INIT
        g_, b_, tt_, lt_, teps = prompt_tail
        _need_gpu(g_, b_, tt_, lt_)
        assert all(t.dtype == _BF16 and t.is_contiguous() for t in (g_, b_, tt_, lt_)) and g_.numel() == b_.numel() == tt_.numel() == 256
        ttab = (ctypes.c_void_p * 4)(g_.data_ptr(), b_.data_ptr(), tt_.data_ptr(), lt_.data_ptr())
        rc = _lib.lib().wg_dec_tokens_ctp_f32(stages, 1 if skip_pe else 0, queries.data_ptr(), query_pe.data_ptr(), _ptr(init_tokens), _ptr(init_prompt),
                                              ttab, float(teps), table, 24, _ptr(q_t2i), _ptr(attn_partials), n_splits, _ptr(mlp_partials),
                                              _ptr(k_i2t), _ptr(v_i2t), P, float(eps), _stream())
        _lib.check(rc, "wg_dec_tokens_ctp_f32")
        return queries
    rc = _lib.lib().wg_dec_tokens_f32(stages, 1 if skip_pe else 0, queries.data_ptr(), query_pe.data_ptr(), _ptr(init_tokens), _ptr(init_prompt),
                                      table, 24, _ptr(q_t2i),
                                      _ptr(attn_partials), n_splits, _ptr(mlp_partials), _ptr(k_i2t), _ptr(v_i2t), P, float(eps), _stream())
    _lib.check(rc, "wg_dec_tokens_f32")
    return queries


def _prompt_image_ok(prompt_image, P, n_images):
    assert prompt_image.dtype == torch.int32 and prompt_image.is_contiguous() and prompt_image.numel() == P and n_images >= 1


def dec_attn_partial(q_t2i, kv_img, prompt_image=None):
    """Token->image attention partials (wg_dec_attn_partial_f32).  q_t2i [P, 6, 128] fp32; kv_img [1 | P, hw, 256] bf16: the projected image
    tokens with the columns ordered [K_h | V_h] for head h = 0..7 (16 + 16 each; a column slice of the fused image-side projection);
    with prompt_image (int32 [P]): kv_img [B, hw, 256] holds one block per IMAGE and prompt p attends to block prompt_image[p]
    -> fp32 [P, 8, ceil(hw / 1024), 108] for the COMBINE step."""
    _need_gpu(q_t2i, kv_img, prompt_image)
    P = q_t2i.shape[0]
    _f32_tokens(q_t2i, P, 128)
    hw = kv_img.shape[1]
    assert kv_img.dtype == _BF16 and kv_img.shape[-1] == 256 and kv_img.stride(-1) == 1
    if prompt_image is not None:
        _prompt_image_ok(prompt_image, P, kv_img.shape[0])
        img_bs = kv_img.stride(0) // kv_img.stride(1) if kv_img.shape[0] > 1 else hw
    else:
        assert kv_img.shape[0] in (1, P)
        img_bs = 0 if kv_img.shape[0] == 1 and P > 1 else (kv_img.stride(0) // kv_img.stride(1) if kv_img.shape[0] > 1 else hw)
    n_splits = (hw + 1023) // 1024
    part = torch.empty(P, 8, n_splits, _TOK_PART, device=q_t2i.device, dtype=torch.float32)
    rc = _lib.lib().wg_dec_attn_partial_f32(q_t2i.data_ptr(), kv_img.data_ptr(), kv_img.data_ptr() + 32, kv_img.stride(1), 32, img_bs,
                                            _ptr(prompt_image), hw, part.data_ptr(), n_splits, P, _stream())
    _lib.check(rc, "wg_dec_attn_partial_f32")
    return part


def _combine_table(combine, P):
    """(attention partials [P, 8, n_splits, 108] fp32, out_proj weight [256, 128], bias, LayerNorm gamma, beta) -> (ctypes table, n_splits)"""
    import ctypes
    if combine is None:
        return None, 0
    part, wo, bo, g, b = combine
    _need_gpu(part, wo, bo, g, b)
    assert part.dtype == torch.float32 and part.is_contiguous() and part.dim() == 4 and part.shape[0] == P and part.shape[1] == 8
    assert part.shape[3] == _TOK_PART and _tiled_ok(wo, 256, 128) and bo.numel() == 256 and g.numel() == 256 and b.numel() == 256
    assert all(t.dtype == _BF16 and t.is_contiguous() for t in (bo, g, b))
    return (ctypes.c_void_p * 5)(part.data_ptr(), wo.data_ptr(), bo.data_ptr(), g.data_ptr(), b.data_ptr()), part.shape[2]


def dec_mlp_slices():
    """Slices the library cuts the decoder MLP's 2048 hidden units into (wg_dec_mlp_slices): lin2 is tiled in that many K-slices."""
    return int(_lib.lib().wg_dec_mlp_slices())


def dec_mlp_partial(x, lin1_w, lin1_b, lin2_w, combine=None, eps=1e-5):
    """The S = dec_mlp_slices() slices of mlp(x) for x [P, 6, 256] fp32 (wg_dec_mlp_partial_f32) -> fp32 [P, S, 6, 256]; lin2's bias is added
    by dec_tokens(TOK_SUM_MLP).  With `combine` (see _combine_table) x holds the tokens before the COMBINE stage, which the launch runs
    itself: returns (partials, tokens after the LayerNorm -- a new buffer)."""
    _need_gpu(x, lin1_w, lin1_b, lin2_w)
    P = x.shape[0]
    _f32_tokens(x, P, 256)
    S = dec_mlp_slices()
    assert _tiled_ok(lin1_w, 2048, 256) and _tiled_ok(lin2_w, 256, 2048, S) and lin1_b.shape == (2048,)     # ops.tile_weight(w), (w, S)
    assert lin1_b.dtype == _BF16 and lin1_b.is_contiguous()
    out = torch.empty(P, S, 6, 256, device=x.device, dtype=torch.float32)
    table, n_splits = _combine_table(combine, P)
    x_out = torch.empty_like(x) if combine is not None else None
    rc = _lib.lib().wg_dec_mlp_partial_f32(x.data_ptr(), table, n_splits, float(eps), _ptr(x_out), lin1_w.data_ptr(), lin1_b.data_ptr(),
                                           lin2_w.data_ptr(), out.data_ptr(), P, _stream())
    _lib.check(rc, "wg_dec_mlp_partial_f32")
    return out if combine is None else (out, x_out)


def dec_heads(x, weights, combine=None, eps=1e-5):
    """The four hypernetwork MLPs and the IoU head on x [P, 6, 256] fp32 (wg_dec_heads_f32); weights: 30 bf16 tensors
    -> (hyper fp32 [P, 4, 32], iou fp32 [P, 4]).  With `combine` the launch first applies the final attention's COMBINE stage."""
    import ctypes
    _need_gpu(x, *weights)
    P = x.shape[0]
    _f32_tokens(x, P, 256)
    assert len(weights) == 30 and all(w.dtype == _BF16 and w.is_contiguous() for w in weights)
    for i in range(5):
        assert all(_tiled_ok(weights[(3 * i + j) * 2], n, 256) for j, n in enumerate((256, 256, 32 if i < 4 else 4))), i
    hyper = torch.empty(P, 4, 32, device=x.device, dtype=torch.float32)
    iou = torch.empty(P, 4, device=x.device, dtype=torch.float32)
    table = (ctypes.c_void_p * 30)(*[w.data_ptr() for w in weights])
    ctab, n_splits = _combine_table(combine, P)
    rc = _lib.lib().wg_dec_heads_f32(x.data_ptr(), ctab, n_splits, float(eps), table, 30, hyper.data_ptr(), iou.data_ptr(), P, _stream())
    _lib.check(rc, "wg_dec_heads_f32")
    return hyper, iou


def dec_i2t_rows(q_img, k_i2t, v_i2t, out_w, out_b, keys, ln_g, ln_b, eps, P, res_bias=None, prompt_image=None):
    """transformer.py:173-180 in one launch (wg_dec_i2t_rows_bf16): norm4(keys + out_proj(attention of every image token over the six
    prompt tokens)).  q_img [1 | P, hw, 128] bf16 (column slice of the image-side projection), k_i2t / v_i2t [P, 6, 128] bf16,
    keys [1 | P, hw, 256] bf16 -> bf16 [P, hw, 256].  res_bias [256] bf16: the residual is keys + res_bias (a constant row the caller
    never added to the image tokens).  prompt_image (int32 [P]): q_img / keys hold one block per IMAGE, prompt p reads block prompt_image[p]."""
    _need_gpu(q_img, k_i2t, v_i2t, out_w, out_b, keys, ln_g, ln_b, res_bias, prompt_image)
    assert res_bias is None or (res_bias.dtype == _BF16 and res_bias.numel() == 256 and res_bias.is_contiguous())
    hw = keys.shape[1]
    assert q_img.dtype == _BF16 and q_img.shape[-1] == 128 and q_img.stride(-1) == 1 and q_img.shape[:2] == keys.shape[:2]
    assert keys.dtype == _BF16 and keys.shape[-1] == 256 and keys.stride(-1) == 1 and (prompt_image is not None or keys.shape[0] in (1, P))
    if prompt_image is not None:
        _prompt_image_ok(prompt_image, P, keys.shape[0])
    assert k_i2t.shape == (P, 6, 128) and v_i2t.shape == (P, 6, 128) and k_i2t.is_contiguous() and v_i2t.is_contiguous()
    assert out_w.shape == (256, 128) and out_w.is_contiguous() and out_b.numel() == 256 and ln_g.numel() == 256 and ln_b.numel() == 256
    for t in (q_img, keys):          # rows of all prompts must be evenly spaced
        assert t.shape[0] == 1 or t.stride(0) == hw * t.stride(1)
    shared = prompt_image is None and keys.shape[0] == 1 and P > 1
    out = torch.empty(P, hw, 256, device=keys.device, dtype=_BF16)
    rc = _lib.lib().wg_dec_i2t_rows_bf16(q_img.data_ptr(), q_img.stride(1), k_i2t.data_ptr(), v_i2t.data_ptr(), out_w.data_ptr(),
                                         out_b.data_ptr(), keys.data_ptr(), keys.stride(1), _ptr(res_bias), hw if shared else 0, _ptr(prompt_image),
                                         ln_g.data_ptr(),
                                         ln_b.data_ptr(), float(eps), out.data_ptr(), P, hw, _stream())
    _lib.check(rc, "wg_dec_i2t_rows_bf16")
    return out


def upscale_mask(keys, up1_w, up1_b, ln_g, ln_b, eps, up2_w, up2_b, hyper, h, w, first_mask, num_masks):
    """mask_decoder.py:140-160 in one launch.  keys [P, h*w, 256] bf16 image tokens; up1_w [(dy,dx,64), 256] (in fragment order,
    ops.tile_weight), up2_w [(dy,dx,32), 64] (re-laid ConvTranspose2d weights); hyper [P, nmask, 32] fp32 -> fp32 [P, num_masks, 4h, 4w]."""
    _need_gpu(keys, up1_w, up1_b, ln_g, ln_b, up2_w, up2_b, hyper)
    P = keys.shape[0]
    assert keys.dtype == _BF16 and keys.is_contiguous() and keys.shape[1:] == (h * w, 256)
    assert _tiled_ok(up1_w, 256, 256) and up2_w.shape == (128, 64) and up2_w.is_contiguous()     # up1_w: ops.tile_weight of the re-laid ConvT
    assert hyper.dtype == torch.float32 and hyper.is_contiguous() and hyper.shape[0] == P and hyper.shape[2] == 32
    masks = torch.empty(P, num_masks, 4 * h, 4 * w, device=keys.device, dtype=torch.float32)
    rc = _lib.lib().wg_upscale_mask_bf16(keys.data_ptr(), 256, up1_w.data_ptr(), up1_b.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(),
                                         float(eps), up2_w.data_ptr(), up2_b.data_ptr(), hyper.data_ptr(), masks.data_ptr(), P, h, w,
                                         hyper.shape[1], first_mask, num_masks, _stream())
    _lib.check(rc, "wg_upscale_mask_bf16")
    return masks


def postprocess_masks(low_res, img_size, input_size, original_size):
    """fp32 [N, C, lh, lw] -> fp32 [N, C, H0, W0] (Sam.postprocess_masks, both resamples + crop in one pass)."""
    _need_gpu(low_res)
    assert low_res.dtype == torch.float32 and low_res.is_contiguous() and low_res.dim() == 4
    N, C, lh, lw = low_res.shape
    out = torch.empty(N, C, int(original_size[0]), int(original_size[1]), device=low_res.device, dtype=torch.float32)
    rc = _lib.lib().wg_postprocess_masks_f32(low_res.data_ptr(), out.data_ptr(), N * C, lh, lw, img_size,
                                             int(input_size[0]), int(input_size[1]), int(original_size[0]),
                                             int(original_size[1]), _stream())
    _lib.check(rc, "wg_postprocess_masks_f32")
    return out


def postprocess_masks_scored(low_res, img_size, input_size, original_size):
    """postprocess_masks for single-channel masks plus their mask scores in the same pass (wg_postprocess_masks_score_f32):
    fp32 [N, 1, lh, lw] -> (fp32 [N, H0, W0], fp32 [N])."""
    _need_gpu(low_res)
    assert low_res.dtype == torch.float32 and low_res.is_contiguous() and low_res.dim() == 4 and low_res.shape[1] == 1
    N, _, lh, lw = low_res.shape
    H0, W0 = int(original_size[0]), int(original_size[1])
    out = torch.empty(N, H0, W0, device=low_res.device, dtype=torch.float32)
    score = torch.empty(N, device=low_res.device, dtype=torch.float32)
    L = _lib.lib()
    nws = L.wg_postprocess_score_workspace_floats(N, H0, W0)
    ws = torch.empty(nws, device=low_res.device, dtype=torch.float32)
    if N <= _SCORE_FUSED_MASKS:
        # one launch: the workgroup that completes a mask folds its partials (tickets: zero words the kernel leaves zero, one set per stream).
        # For the few masks of one image's decode, where the chain is latency (-1.3 us of 200); with a batch's masks the fat workgroups of
        # the fused form cost more than the second launch (8 masks: 19 against 15 us), so those keep the two-launch form
        rc = L.wg_postprocess_masks_score_fused_f32(low_res.data_ptr(), out.data_ptr(), score.data_ptr(), ws.data_ptr(), nws,
                                                    _score_tickets(low_res.device).data_ptr(), N, lh, lw, img_size, int(input_size[0]),
                                                    int(input_size[1]), H0, W0, _stream())
        _lib.check(rc, "wg_postprocess_masks_score_fused_f32")
        return out, score
    rc = L.wg_postprocess_masks_score_f32(low_res.data_ptr(), out.data_ptr(), score.data_ptr(), ws.data_ptr(), nws, N, lh, lw, img_size,
                                          int(input_size[0]), int(input_size[1]), H0, W0, _stream())
    _lib.check(rc, "wg_postprocess_masks_score_f32")
    return out, score


_SCORE_TICKETS = 64
_SCORE_FUSED_MASKS = 4
_score_ticket_cache = {}
_score_ticket_pool = {}
_score_ticket_keep = []      # every set ever handed to a capture: a captured graph bakes in the raw address, so the storage lives as long as the process


def _score_tickets(device):
    """Zero words for wg_postprocess_masks_score_fused_f32 (the kernel leaves them zero).  Eager calls share one set per (device, stream): launches on
    one HIP stream are ordered, which is all that sharing needs.  A call made under stream CAPTURE gets a set of its own: the graph is replayed on
    whatever stream is current then, possibly beside eager calls on a stream whose pooled handle equals the capture stream's, and two launches adding
    to the same words misdetect the last arriver.  The sets for captures come from a small pool zeroed eagerly on the first eager call (no memset node
    in the latency-bound decode graph); a capture that finds the pool empty allocates inside the capture (a memset node, replayed with the graph).
    The caller only takes data_ptr(): every set handed to a capture is therefore parked in _score_ticket_keep (views keep their whole block alive), or the
    caching allocator would hand the words to a later tensor while replayed graphs still count arrivals in them."""
    if torch.cuda.is_current_stream_capturing():
        pool = _score_ticket_pool.get(device.index)
        t = pool.pop() if pool else torch.zeros(_SCORE_TICKETS, device=device, dtype=torch.int32)
        _score_ticket_keep.append(t)
        return t
    if device.index not in _score_ticket_pool:
        _score_ticket_pool[device.index] = list(torch.zeros(16, _SCORE_TICKETS, device=device, dtype=torch.int32).unbind(0))
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _score_ticket_cache.get(key)
    if t is None:
        t = _score_ticket_cache[key] = torch.zeros(_SCORE_TICKETS, device=device, dtype=torch.int32)
    return t


def mask_score(masks):
    """fp32 [N, H, W] -> fp32 [N]."""
    _need_gpu(masks)
    assert masks.dtype == torch.float32 and masks.is_contiguous()
    N = masks.shape[0]
    hw = masks.numel() // N
    score = torch.empty(N, device=masks.device, dtype=torch.float32)
    nws = _lib.lib().wg_mask_score_workspace_floats(N, hw)
    ws = torch.empty(nws, device=masks.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_mask_score_f32(masks.data_ptr(), score.data_ptr(), ws.data_ptr(), nws, N, hw, _stream()), "wg_mask_score_f32")
    return score


def avgpool_tokens(x, B, H, W, s):
    """channels-last [B,H,W,C] rows -> [B, (H/s)*(W/s), C]."""
    _need_gpu(x)
    C = x.shape[-1]
    assert x.is_contiguous() and x.dtype == _BF16 and x.numel() == B * H * W * C
    y = torch.empty(B, (H // s) * (W // s), C, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_avgpool_tokens_bf16(x.data_ptr(), y.data_ptr(), B, H, W, C, s, _stream()), "wg_avgpool_tokens_bf16")
    return y


def mean_tokens(x):
    """[B, L, C] -> [B, 1, C]."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == _BF16 and x.dim() == 3
    B, L, C = x.shape
    y = torch.empty(B, 1, C, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_mean_tokens_bf16(x.data_ptr(), y.data_ptr(), B, L, C, _stream()), "wg_mean_tokens_bf16")
    return y


def sigmoid_gate(x, logit):
    """x [..., C] bf16 * sigmoid(logit [...]) fp32."""
    _need_gpu(x, logit)
    assert x.is_contiguous() and logit.is_contiguous() and logit.dtype == torch.float32
    C = x.shape[-1]
    rows = x.numel() // C
    assert logit.numel() == rows
    y = torch.empty(x.shape, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_sigmoid_gate_bf16(x.data_ptr(), logit.data_ptr(), y.data_ptr(), rows, C, _stream()), "wg_sigmoid_gate_bf16")
    return y


def ctp_tail(x, gamma, beta, text_type, log_temp, eps):
    """normalize(LayerNorm(x) + text_type, dim=-1) * exp(log_temp)."""
    _need_gpu(x, gamma, beta, text_type, log_temp)
    M, C, ldx = _rows(x)
    y = torch.empty(x.shape, device=x.device, dtype=_BF16)
    _, _, ldy = _rows(y)
    rc = _lib.lib().wg_ctp_tail_bf16(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), text_type.data_ptr(),
                                     log_temp.data_ptr(), y.data_ptr(), ldy, M, C, float(eps), _stream())
    _lib.check(rc, "wg_ctp_tail_bf16")
    return y


def resample_tokens(x, target=16):
    """[n, p*p, C] -> bilinear (align_corners=False) -> [n, target*target, C]."""
    _need_gpu(x)
    assert x.is_contiguous() and x.dtype == _BF16 and x.dim() == 3
    n, l, C = x.shape
    p = int(round(l ** 0.5))
    assert p * p == l, "Token count %d is not square." % l
    y = torch.empty(n, target * target, C, device=x.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_resample_tokens_bf16(x.data_ptr(), y.data_ptr(), n, p, target, C, _stream()), "wg_resample_tokens_bf16")
    return y


def mask_iou(pred_logits, gt, ignore_index=255):
    """intersectionAndUnionGPU(pred > 0, gt, K=2, ignore_index) per mask, thresholding fused.  pred_logits, gt fp32 [N,H,W]
    (gt values 0 / 1 / ignore_index) -> (intersection [N,2], union [N,2], target_area [N,2]) fp32."""
    _need_gpu(pred_logits, gt)
    assert pred_logits.dtype == torch.float32 and gt.dtype == torch.float32 and pred_logits.shape == gt.shape
    assert pred_logits.is_contiguous() and gt.is_contiguous()
    N = pred_logits.shape[0]
    hw = pred_logits.numel() // N
    out = torch.empty(N, 6, device=pred_logits.device, dtype=torch.float32)
    nws = _lib.lib().wg_mask_stats_workspace_floats(N, hw)
    ws = torch.empty(nws, device=pred_logits.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_mask_iou_f32(pred_logits.data_ptr(), gt.data_ptr(), out.data_ptr(), ws.data_ptr(), nws, N, hw,
                                          float(ignore_index), _stream()), "wg_mask_iou_f32")
    return out[:, 0:2], out[:, 2:4], out[:, 4:6]


def mask_losses(pred_logits, targets, num_masks, dice_scale=1000.0, dice_eps=1e-6):
    """(sigmoid_ce_loss, dice_loss) forward of utils_walkgpt.py:76-120: per-mask reductions on the GPU, the final
    sum / (num_masks + 1e-8) over N scalars on the host side of the stream (torch, N values)."""
    _need_gpu(pred_logits, targets)
    assert pred_logits.dtype == torch.float32 and targets.dtype == torch.float32 and pred_logits.shape == targets.shape
    assert pred_logits.is_contiguous() and targets.is_contiguous()
    N = pred_logits.shape[0]
    hw = pred_logits.numel() // N
    out = torch.empty(N, 2, device=pred_logits.device, dtype=torch.float32)
    nws = _lib.lib().wg_mask_stats_workspace_floats(N, hw)
    ws = torch.empty(nws, device=pred_logits.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_mask_losses_f32(pred_logits.data_ptr(), targets.data_ptr(), out.data_ptr(), ws.data_ptr(), nws, N, hw,
                                             float(dice_scale), float(dice_eps), _stream()), "wg_mask_losses_f32")
    per = out.sum(0) / (num_masks + 1e-8)
    return per[0], per[1]


def nce_forward(z, sam_tokens, seg_row_ids, wq, bq, wk_t, temperature, top_k, exclude_same_row, want_logits=False):
    """Device part of infonce_loss() (utils_walkgpt.py:8-73) for normalize=True.

    z [M, D] bf16 [SEG] embeddings; sam_tokens [rows, N, D] bf16; seg_row_ids [M] int; wq/bq the query projection of
    TinyCrossAttn and wk_t = Wk^T (contiguous [D, D]): q.(Wk kv) = (Wk^T q).kv.  Returns a dict with the fp32 GEMM `st`,
    `inv_norm`, `zn`, `attn_w` [M, N], `vraw` [M, D] (top-k refined positive, or the attention-pooled raw token when the
    refinement is off) and a `finish(vpos)` closure producing (loss, loss_m, logits)."""
    _need_gpu(z, sam_tokens, seg_row_ids)
    assert z.dtype == _BF16 and sam_tokens.dtype == _BF16 and sam_tokens.is_contiguous() and z.dim() == 2
    rows, N, D = sam_tokens.shape
    M = z.shape[0]
    assert z.shape[1] == D and seg_row_ids.shape == (M,)
    dev = z.device
    L = _lib.lib()
    tok2 = sam_tokens.reshape(rows * N, D)
    seg = seg_row_ids.to(torch.int32).contiguous()
    zc = z.contiguous()
    qcat = torch.empty(2 * M, D, device=dev, dtype=_BF16)
    _lib.check(L.wg_l2_normalize_rows_bf16(zc.data_ptr(), D, qcat.data_ptr(), D, M, D, 1e-12, _stream()), "wg_l2_normalize_rows_bf16")
    q = linear(zc, wq, bq)                       # [M, D]   TinyCrossAttn.wq
    linear(q, wk_t, out=qcat[M:])                # rows M..2M-1: Wk^T q
    inv_norm = torch.empty(rows * N, device=dev, dtype=torch.float32)
    _lib.check(L.wg_row_inv_norm_bf16(tok2.data_ptr(), D, inv_norm.data_ptr(), rows * N, D, 1e-12, _stream()), "wg_row_inv_norm_bf16")
    st = linear(qcat, tok2, out_f32=True)        # [2M, rows*N] fp32
    attn_w = torch.empty(M, N, device=dev, dtype=torch.float32)
    vraw = torch.empty(M, D, device=dev, dtype=torch.float32)
    k = int(top_k) if (top_k is not None and 0 < top_k < N) else 0
    _lib.check(L.wg_nce_attn_f32(st.data_ptr(), st.stride(0), tok2.data_ptr(), D, seg.data_ptr(), attn_w.data_ptr(), vraw.data_ptr(),
                                 M, N, rows, D, k if k <= 32 else 0, float(D) ** -0.5, _stream()), "wg_nce_attn_f32")
    if k > 32:
        # beyond the attention kernel's in-register selection: pick the k tokens from its weights and pool them with the streaming kernel
        # (weights renormalised over the selection = the softmax of their scores, utils_walkgpt.py:37-40)
        idx = torch.topk(attn_w, k=k, dim=1).indices
        kt = torch.gather(sam_tokens.index_select(0, seg_row_ids.long()), 1, idx.unsqueeze(-1).expand(-1, -1, D)).contiguous()
        vb = torch.empty(M, D, device=dev, dtype=_BF16)
        _lib.check(L.wg_pool_rows_bf16(qcat[M:].data_ptr(), kt.data_ptr(), None, vb.data_ptr(), M, k, D, _stream()), "wg_pool_rows_bf16")
        vraw = vb.float()

    def finish(vpos):
        assert vpos.dtype == torch.float32 and vpos.is_contiguous() and vpos.shape == (M, D)
        loss_m = torch.empty(M, device=dev, dtype=torch.float32)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        logits = torch.empty(M, 1 + rows * N, device=dev, dtype=torch.float32) if want_logits else None
        _lib.check(L.wg_nce_loss_f32(st.data_ptr(), st.stride(0), inv_norm.data_ptr(), qcat.data_ptr(), vpos.data_ptr(), seg.data_ptr(),
                                     loss_m.data_ptr(), loss.data_ptr(), _ptr(logits), M, N, rows, D, 1 if exclude_same_row else 0,
                                     float(temperature), _stream()), "wg_nce_loss_f32")
        return loss[0], loss_m, logits

    return {"st": st, "inv_norm": inv_norm, "zn": qcat[:M], "attn_w": attn_w, "vraw": vraw, "refined": k > 0, "finish": finish}


def match_cost(pred_logits, targets, point_coords):
    """[P, T] matching cost of utils/matcher.py:93-133 (point-sampled BCE + dice).  pred_logits [P,H,W], targets [T,H,W]
    fp32, point_coords [NP, 2] fp32 in [0,1]^2 as (x, y)."""
    _need_gpu(pred_logits, targets, point_coords)
    assert pred_logits.dtype == torch.float32 and targets.dtype == torch.float32 and point_coords.dtype == torch.float32
    assert pred_logits.is_contiguous() and targets.is_contiguous() and point_coords.is_contiguous()
    P, H, W = pred_logits.shape
    T = targets.shape[0]
    assert targets.shape[1:] == (H, W) and point_coords.dim() == 2 and point_coords.shape[1] == 2
    NP = point_coords.shape[0]
    cost = torch.empty(P, T, device=pred_logits.device, dtype=torch.float32)
    nws = _lib.lib().wg_match_cost_workspace_floats(P, T, NP)
    ws = torch.empty(nws, device=pred_logits.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_match_cost_f32(pred_logits.data_ptr(), targets.data_ptr(), point_coords.data_ptr(), cost.data_ptr(),
                                            ws.data_ptr(), nws, P, T, H, W, NP, _stream()), "wg_match_cost_f32")
    return cost


# ---- SamAutomaticMaskGenerator behind the decoder (csrc/amg.hip) ---------------------------------------------------------------------------
def amg_mask_stats(low_res, img_size, input_size, original_size, thr, offset):
    """Low-res logits fp32 [N, lh, lw] -> (stats int32 [N, 8], bits int32 [N, ceil(H0 / 32), W0]) of the masks Sam.postprocess_masks would give,
    without writing them (wg_amg_mask_stats_f32): stats = {count(x > thr + offset), count(x > thr - offset), count(x > thr), x_min, y_min, x_max,
    y_max, 0}, the box as batched_mask_to_box (amg.py:303-346); bit r of bits[n, yb, x] = (pixel (32 yb + r, x) > thr).  (The words are the
    kernel's uint32 in an int32 tensor: torch has no arithmetic on uint32.)"""
    _need_gpu(low_res)
    assert low_res.dtype == torch.float32 and low_res.is_contiguous() and low_res.dim() == 3
    N, lh, lw = low_res.shape
    H0, W0 = int(original_size[0]), int(original_size[1])
    stats = torch.empty(N, 8, device=low_res.device, dtype=torch.int32)
    bits = torch.empty(N, (H0 + 31) // 32, W0, device=low_res.device, dtype=torch.int32)
    L = _lib.lib()
    nws = L.wg_amg_mask_stats_workspace_ints(N, H0, W0)
    ws = torch.empty(nws, device=low_res.device, dtype=torch.int32)
    rc = L.wg_amg_mask_stats_f32(low_res.data_ptr(), stats.data_ptr(), bits.data_ptr(), ws.data_ptr(), nws, N, lh, lw, int(img_size),
                                 int(input_size[0]), int(input_size[1]), H0, W0, float(thr), float(offset), _stream())
    _lib.check(rc, "wg_amg_mask_stats_f32")
    return stats, bits


def rle_from_positions(positions, ends, first, size):
    """The host half of amg_rle: sorted change positions of all masks (one int array), `ends` = where each mask's run of them stops, first[k] =
    the mask's bit 0 -> the uncompressed RLEs of mask_to_rle_pytorch (amg.py:120-135): the runs are the differences of [0, positions.., H W],
    with a leading 0 when the mask starts set.  numpy only; one np.diff per mask, no loop over runs or pixels."""
    import numpy as np
    H, W = int(size[0]), int(size[1])
    out, start = [], 0
    for k, end in enumerate(np.asarray(ends).tolist()):
        edges = np.empty(end - start + 2, dtype=np.int64)
        edges[0], edges[-1] = 0, H * W
        edges[1:-1] = positions[start:end]
        runs = np.diff(edges).tolist()
        out.append({"size": [H, W], "counts": ([0] + runs) if first[k] else runs})
        start = end
    return out


def amg_rle(bits, keep, crop_box, frame_size):
    """Uncompressed RLEs (mask_to_rle_pytorch of uncrop_masks, amg.py:107-135, :255-264) of the bit planes bits[keep[k]] (amg_mask_stats's layout),
    each placed at crop_box = [x0, y0, x1, y1] of an (H, W) frame: a list of {"size": [H, W], "counts": [...]}.  `keep`: int32 / int64 indices
    on the device, every one in [0, N) (checked).  Count pass, one scan (torch.cumsum), one blocking read of its total (with the range check of
    `keep`) before the write pass, then the blocking copies of the positions, the per-mask totals and the first bits to the host."""
    _need_gpu(bits, keep)
    assert bits.dtype == torch.int32 and bits.is_contiguous() and bits.dim() == 3
    assert keep.dim() == 1 and keep.dtype in (torch.int32, torch.int64)
    H, W = int(frame_size[0]), int(frame_size[1])
    x0, y0, x1, y1 = (int(v) for v in crop_box)
    N, hb, out_w = bits.shape
    out_h = y1 - y0
    assert out_w == x1 - x0 and hb == (out_h + 31) // 32, "bits %s do not belong to crop box %s" % (tuple(bits.shape), list(crop_box))
    K = keep.shape[0]
    if K == 0:
        return []
    keep = keep.to(torch.int32).contiguous()
    L = _lib.lib()
    counts = torch.empty(K, out_w, device=bits.device, dtype=torch.int32)
    _lib.check(L.wg_amg_rle_count_i32(bits.data_ptr(), keep.data_ptr(), counts.data_ptr(), N, K, out_h, out_w, x0, y0, H, W, _stream()),
               "wg_amg_rle_count_i32")
    offsets = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    # (the kernels clamp an index outside the planes instead of reading there; the list is judged with the read of the total)
    total, bad = torch.stack([offsets[-1], ((keep < 0) | (keep >= N)).sum()]).tolist()
    if bad:
        raise _lib.WalkgptHipError("amg_rle: %d of the %d indices in `keep` lie outside the %d bit planes" % (bad, K, N))
    positions = torch.empty(max(total, 1), device=bits.device, dtype=torch.int32)
    first = torch.empty(K, device=bits.device, dtype=torch.int32)
    _lib.check(L.wg_amg_rle_write_i32(bits.data_ptr(), keep.data_ptr(), offsets.data_ptr(), positions.data_ptr(), total, first.data_ptr(), N, K,
                                      out_h, out_w, x0, y0, H, W, _stream()), "wg_amg_rle_write_i32")
    ends = offsets.reshape(K, out_w)[:, -1]
    return rle_from_positions(positions[:total].cpu().numpy(), ends.cpu().numpy(), first.cpu().numpy(), (H, W))


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms (one category, which is how automatic_mask_generator.py calls batched_nms): boxes [N, 4] XYXY, scores [N] -> int64
    indices of the kept boxes by descending score (wg_nms_f32).  The order is a stable descending sort: equal scores keep their input order."""
    _need_gpu(boxes, scores)
    assert boxes.dim() == 2 and boxes.shape[1] == 4 and scores.shape == (boxes.shape[0],)
    N = boxes.shape[0]
    if N == 0:
        return torch.empty(0, device=boxes.device, dtype=torch.int64)
    boxes = boxes.float().contiguous()
    order = torch.sort(scores, descending=True, stable=True)[1].to(torch.int32)
    keep = torch.empty(N, device=boxes.device, dtype=torch.int32)
    n_keep = torch.empty(1, device=boxes.device, dtype=torch.int32)
    L = _lib.lib()
    nws = L.wg_nms_workspace_words(N)
    ws = torch.empty(nws, device=boxes.device, dtype=torch.int64)
    _lib.check(L.wg_nms_f32(boxes.data_ptr(), order.data_ptr(), float(iou_threshold), keep.data_ptr(), n_keep.data_ptr(), ws.data_ptr(), nws, N,
                            _stream()), "wg_nms_f32")
    return keep[:int(n_keep.item())].to(torch.int64)


# ---- the LLaMA generate path (csrc/llama.hip): thin wrappers, no allocation unless `out` is missing (they run inside a graph capture) ----------
def rmsnorm(x, weight, eps, out=None, slot=None, slot_add=0):
    """y = x * rsqrt(mean(x^2) + eps) * weight per row (wg_rmsnorm_rows_bf16).  slot (int32 [1] on the device): `out` is [rows, slot_cap, D] and
    row r is written to out[r, clamp(slot + slot_add)]."""
    _need_gpu(x, weight, out, slot)
    assert x.dtype == _BF16 and weight.dtype == _BF16
    M, D, ldx = _rows(x)
    if out is None:
        assert slot is None
        out = torch.empty(x.shape, device=x.device, dtype=_BF16)
    if slot is None:
        Mo, Do, ldy = _rows(out)
        assert (Mo, Do) == (M, D)
        slot_cap, ybs = 0, 0
    else:
        assert out.dim() == 3 and out.is_contiguous() and out.shape[0] == M and out.shape[2] == D and slot.dtype == torch.int32
        slot_cap, ldy, ybs = out.shape[1], D, out.stride(0)
    _lib.check(_lib.lib().wg_rmsnorm_rows_bf16(x.data_ptr(), ldx, weight.data_ptr(), out.data_ptr(), ldy, M, D, float(eps), _ptr(slot), int(slot_add),
                                               slot_cap, ybs, _stream()), "wg_rmsnorm_rows_bf16")
    return out


def _lora_rank(mats, rank_axis, other, t):
    """The common rank of the adapter matrices given (None = no adapter on that segment); with none given, t's third of a row, else 8."""
    ranks = {int(m.shape[rank_axis]) for m in mats if m is not None}
    assert len(ranks) <= 1, "one LoRA rank per call"
    for m in mats:
        assert m is None or (m.dtype == _BF16 and m.dim() == 2 and m.is_contiguous() and m.shape[1 - rank_axis] == other)
    if ranks:
        return ranks.pop()
    return int(t.shape[1]) // 3 if t is not None else 8


def llama_rope_cache(qkv, cos, sin, past_len, q_out, k_cache, v_cache, rows, L, heads, t=None, lora_b=None, lora_scale=None):
    """qkv [rows * L, 3H] -> rotated q in q_out [rows * L, H], rotated k and v into k_cache / v_cache [rows, cap, H] at positions past_len + j.
    lora_b = (B_q, B_k, B_v), each [H, r] bf16 or None, lora_scale their three scalings and t fp32 [rows * L, 3 r] (llama_gemv's t_out): the
    adapted ones become x + scale * B t before the rotation (wg_llama_rope_cache_lora_bf16); lora_b None is the plain entry point."""
    _need_gpu(qkv, cos, sin, past_len, q_out, k_cache, v_cache)
    H = heads * 128
    assert qkv.dtype == _BF16 and qkv.shape == (rows * L, 3 * H) and q_out.shape == (rows * L, H) and q_out.dtype == _BF16
    assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape[1] == 64 and sin.shape == cos.shape and sin.is_contiguous()
    assert past_len.dtype == torch.int32
    assert k_cache.is_contiguous() and k_cache.dtype == _BF16 and k_cache.shape[0] == rows and k_cache.shape[2] == H and v_cache.shape == k_cache.shape
    if lora_b is None:
        assert t is None and lora_scale is None
        _lib.check(_lib.lib().wg_llama_rope_cache_bf16(qkv.data_ptr(), qkv.stride(0), cos.data_ptr(), sin.data_ptr(), cos.shape[0], past_len.data_ptr(),
                                                       q_out.data_ptr(), q_out.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), rows, L, heads,
                                                       k_cache.shape[1], _stream()), "wg_llama_rope_cache_bf16")
        return q_out
    lora_b = list(lora_b)
    assert len(lora_b) == 3
    _need_gpu(t, *lora_b)
    rank = _lora_rank(lora_b, 1, H, t)
    scale = [0.0 if b is None else float(sc) for b, sc in zip(lora_b, lora_scale or (0.0, 0.0, 0.0))]
    assert t is None or (t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape == (rows * L, 3 * rank))
    assert t is not None or all(b is None for b in lora_b)
    _lib.check(_lib.lib().wg_llama_rope_cache_lora_bf16(qkv.data_ptr(), qkv.stride(0), cos.data_ptr(), sin.data_ptr(), cos.shape[0], past_len.data_ptr(),
                                                        q_out.data_ptr(), q_out.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), rows, L, heads,
                                                        k_cache.shape[1], _ptr(t), 0 if t is None else t.stride(0), _ptr(lora_b[0]), _ptr(lora_b[1]),
                                                        _ptr(lora_b[2]), scale[0], scale[1], scale[2], rank, _stream()),
               "wg_llama_rope_cache_lora_bf16")
    return q_out


def _llama_cache_args(q, k_cache, v_cache, mask, past_len, heads):
    _need_gpu(q, k_cache, v_cache, mask, past_len)
    rows, cap, H = k_cache.shape
    assert H == heads * 128 and q.dtype == _BF16 and k_cache.dtype == _BF16 and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert v_cache.shape == k_cache.shape and mask.dtype == torch.uint8 and mask.shape == (rows, cap) and mask.is_contiguous()
    assert past_len.dtype == torch.int32
    return rows, cap, H


def llama_attn_prefill(q, k_cache, v_cache, mask, past_len, L, heads, scale, out=None):
    """Causal + key-mask attention of q [rows * L, H] over the cache (query j at position past_len + j)."""
    rows, cap, H = _llama_cache_args(q, k_cache, v_cache, mask, past_len, heads)
    assert q.shape == (rows * L, H)
    if out is None:
        out = torch.empty(rows * L, H, device=q.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_llama_attn_prefill_bf16(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), mask.data_ptr(),
                                                     out.data_ptr(), out.stride(0), past_len.data_ptr(), rows, L, heads, cap, float(scale),
                                                     _stream()), "wg_llama_attn_prefill_bf16")
    return out


def llama_attn_decode_workspace(rows, heads, device):
    return torch.empty(_lib.lib().wg_llama_attn_decode_workspace_floats(rows, heads), device=device, dtype=torch.float32)


def llama_attn_decode(q, k_cache, v_cache, mask, past_len, heads, scale, workspace=None, out=None):
    """One query per row, q [rows, H], over keys 0 .. past_len of the cache."""
    rows, cap, H = _llama_cache_args(q, k_cache, v_cache, mask, past_len, heads)
    assert q.shape == (rows, H)
    if workspace is None:
        workspace = llama_attn_decode_workspace(rows, heads, q.device)
    if out is None:
        out = torch.empty(rows, H, device=q.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_llama_attn_decode_bf16(q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(), mask.data_ptr(),
                                                    workspace.data_ptr(), workspace.numel(), out.data_ptr(), out.stride(0), past_len.data_ptr(),
                                                    rows, heads, cap, float(scale), _stream()), "wg_llama_attn_decode_bf16")
    return out


def llama_quantize_weight(weight):
    """weight [N, K] bf16 contiguous (K % 16 == 0) -> (q uint8 [N, K], the OCP e4m3 bytes, and scale fp32 [N], a power of two per row):
    wg_llama_quantize_weight_e4m3, the format at include/walkgpt_hip.h.  Bit-exact."""
    _need_gpu(weight)
    assert weight.dtype == _BF16 and weight.dim() == 2 and weight.is_contiguous()
    N, K = weight.shape
    q = torch.empty(N, K, device=weight.device, dtype=torch.uint8)
    scale = torch.empty(N, device=weight.device, dtype=torch.float32)
    _lib.check(_lib.lib().wg_llama_quantize_weight_e4m3(weight.data_ptr(), q.data_ptr(), scale.data_ptr(), N, K, _stream()),
               "wg_llama_quantize_weight_e4m3")
    return q, scale


def llama_dequantize_weight(q, scale, out=None):
    """(q uint8 [N, K], scale fp32 [N]) of llama_quantize_weight -> W' = q * scale as bf16 [N, K], exact (wg_llama_dequantize_weight_bf16)."""
    _need_gpu(q, scale, out)
    assert q.dtype == torch.uint8 and q.dim() == 2 and q.is_contiguous()
    N, K = q.shape
    assert scale.dtype == torch.float32 and scale.shape == (N,) and scale.is_contiguous()
    if out is None:
        out = torch.empty(N, K, device=q.device, dtype=_BF16)
    assert out.dtype == _BF16 and out.shape == (N, K) and out.is_contiguous()
    _lib.check(_lib.lib().wg_llama_dequantize_weight_bf16(q.data_ptr(), scale.data_ptr(), out.data_ptr(), N, K, _stream()),
               "wg_llama_dequantize_weight_bf16")
    return out


def llama_gemv(x, weights, gamma=None, eps=0.0, residual=None, out=None, out_f32=False, pair=False, lora_a=None, t_out=None, scales=None):
    """x [M <= 8, K] against one to three weights [N_i, K] whose outputs sit side by side in `out` [M, sum N_i] (pair: silu(W_0 x) * (W_1 x),
    [M, N_0]).  gamma: RMSNorm prologue; residual: added before the rounding (may be `out`).
    lora_a: per weight an adapter down-projection [r, K] bf16 or None; their products with the same (normalised) input go, fp32, into
    t_out [M, 3 r], column block i for weight i, in the same launch (wg_llama_gemv_lora_bf16).  lora_a None is the plain entry point.
    scales: the weights are llama_quantize_weight's e4m3 bytes (uint8) and scales[i] fp32 [N_i] their row scales (wg_llama_gemv_e4m3,
    wg_llama_gemv_lora_e4m3); None: bf16 weights."""
    weights = list(weights)
    _need_gpu(x, gamma, residual, out, *weights)
    assert x.dtype == _BF16 and 1 <= len(weights) <= 3
    M, K, ldx = _rows(x)
    if scales is not None:
        return _llama_gemv_e4m3(x, weights, list(scales), gamma, eps, residual, out, out_f32, pair, lora_a, t_out)
    for w in weights:
        assert w.dtype == _BF16 and w.dim() == 2 and w.shape[1] == K and w.is_contiguous()
    ns = [int(w.shape[0]) for w in weights] + [0] * (3 - len(weights))
    N = ns[0] if pair else sum(ns)
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32 if out_f32 else _BF16)
    Mo, No, ldo = _rows(out)
    assert (Mo, No) == (M, N) and out.dtype == (torch.float32 if out_f32 else _BF16)
    assert gamma is None or (gamma.dtype == _BF16 and gamma.numel() == K and gamma.is_contiguous())
    assert residual is None or residual.shape[-1] == N
    ptrs = [w.data_ptr() for w in weights] + [0] * (3 - len(weights))
    if lora_a is None:
        assert t_out is None
        _lib.check(_lib.lib().wg_llama_gemv_bf16(x.data_ptr(), ldx, ptrs[0], ns[0], ptrs[1], ns[1], ptrs[2], ns[2], K, _ptr(gamma), float(eps),
                                                 _ptr(residual), _residual_ld(residual), out.data_ptr(), ldo, 1 if out_f32 else 0, 1 if pair else 0, M,
                                                 _stream()), "wg_llama_gemv_bf16")
        return out
    lora_a = list(lora_a) + [None] * (3 - len(lora_a))
    assert len(lora_a) == 3
    _need_gpu(t_out, *lora_a)
    rank = _lora_rank(lora_a, 0, K, t_out)
    assert t_out is None or (t_out.dtype == torch.float32 and t_out.dim() == 2 and t_out.stride(1) == 1 and t_out.shape == (M, 3 * rank))
    assert t_out is not None or all(a is None for a in lora_a)
    _lib.check(_lib.lib().wg_llama_gemv_lora_bf16(x.data_ptr(), ldx, ptrs[0], ns[0], ptrs[1], ns[1], ptrs[2], ns[2], K, _ptr(gamma), float(eps),
                                                  _ptr(residual), _residual_ld(residual), out.data_ptr(), ldo, 1 if out_f32 else 0,
                                                  1 if pair else 0, M, _ptr(lora_a[0]), _ptr(lora_a[1]), _ptr(lora_a[2]), rank, _ptr(t_out),
                                                  0 if t_out is None else t_out.stride(0), _stream()), "wg_llama_gemv_lora_bf16")
    return out


def _llama_gemv_e4m3(x, weights, scales, gamma, eps, residual, out, out_f32, pair, lora_a, t_out):
    """llama_gemv's byte-weight form (its checks on x, gamma and residual are done)."""
    _need_gpu(*scales)
    M, K, ldx = _rows(x)
    assert len(scales) == len(weights)
    for w, s in zip(weights, scales):
        assert w.dtype == torch.uint8 and w.dim() == 2 and w.shape[1] == K and w.is_contiguous()
        assert s.dtype == torch.float32 and s.shape == (w.shape[0],) and s.is_contiguous()
    ns = [int(w.shape[0]) for w in weights] + [0] * (3 - len(weights))
    N = ns[0] if pair else sum(ns)
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32 if out_f32 else _BF16)
    Mo, No, ldo = _rows(out)
    assert (Mo, No) == (M, N) and out.dtype == (torch.float32 if out_f32 else _BF16)
    assert gamma is None or (gamma.dtype == _BF16 and gamma.numel() == K and gamma.is_contiguous())
    assert residual is None or residual.shape[-1] == N
    ptrs = [w.data_ptr() for w in weights] + [0] * (3 - len(weights))
    sp = [s.data_ptr() for s in scales] + [0] * (3 - len(scales))
    if lora_a is None:
        assert t_out is None
        _lib.check(_lib.lib().wg_llama_gemv_e4m3(x.data_ptr(), ldx, ptrs[0], sp[0], ns[0], ptrs[1], sp[1], ns[1], ptrs[2], sp[2], ns[2], K,
                                                 _ptr(gamma), float(eps), _ptr(residual), _residual_ld(residual), out.data_ptr(), ldo,
                                                 1 if out_f32 else 0, 1 if pair else 0, M, _stream()), "wg_llama_gemv_e4m3")
        return out
    lora_a = list(lora_a) + [None] * (3 - len(lora_a))
    assert len(lora_a) == 3
    _need_gpu(t_out, *lora_a)
    rank = _lora_rank(lora_a, 0, K, t_out)
    assert t_out is None or (t_out.dtype == torch.float32 and t_out.dim() == 2 and t_out.stride(1) == 1 and t_out.shape == (M, 3 * rank))
    assert t_out is not None or all(a is None for a in lora_a)
    _lib.check(_lib.lib().wg_llama_gemv_lora_e4m3(x.data_ptr(), ldx, ptrs[0], sp[0], ns[0], ptrs[1], sp[1], ns[1], ptrs[2], sp[2], ns[2], K,
                                                  _ptr(gamma), float(eps), _ptr(residual), _residual_ld(residual), out.data_ptr(), ldo,
                                                  1 if out_f32 else 0, 1 if pair else 0, M, _ptr(lora_a[0]), _ptr(lora_a[1]), _ptr(lora_a[2]),
                                                  rank, _ptr(t_out), 0 if t_out is None else t_out.stride(0), _stream()),
               "wg_llama_gemv_lora_e4m3")
    return out


def llama_silu_mul(gate_up, out=None):
    """gate_up [M, 2I] (gate | up) -> silu(gate) * up [M, I]."""
    _need_gpu(gate_up, out)
    assert gate_up.dtype == _BF16
    M, I2, ld = _rows(gate_up)
    if out is None:
        out = torch.empty(M, I2 // 2, device=gate_up.device, dtype=_BF16)
    _lib.check(_lib.lib().wg_llama_silu_mul_bf16(gate_up.data_ptr(), ld, out.data_ptr(), _rows(out)[2], M, I2 // 2, _stream()),
               "wg_llama_silu_mul_bf16")
    return out


def llama_pick_token(logits, embed, x_next, tokens, finished, mask, state, eos, pad):
    """The greedy step on the device (wg_llama_pick_token): logits fp32 [rows, V], embed bf16 [>= V, H], x_next bf16 [rows, H], tokens int64
    [rows, tok_cap], finished int32 [rows], mask uint8 [rows, cap], state int32 {past_len, n_new}.  eos None: no eos / pad rule."""
    _need_gpu(logits, embed, x_next, tokens, finished, mask, state)
    rows, V = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and embed.dtype == _BF16 and embed.is_contiguous()
    assert x_next.dtype == _BF16 and x_next.shape == (rows, embed.shape[1]) and tokens.dtype == torch.int64 and tokens.is_contiguous()
    assert finished.dtype == torch.int32 and finished.numel() == rows and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape[0] == rows
    assert state.dtype == torch.int32 and state.numel() >= 2 and tokens.shape[0] == rows
    _lib.check(_lib.lib().wg_llama_pick_token(logits.data_ptr(), logits.stride(0), embed.data_ptr(), embed.shape[0], x_next.data_ptr(),
                                              x_next.stride(0), tokens.data_ptr(), tokens.shape[1], finished.data_ptr(), mask.data_ptr(),
                                              state.data_ptr(), -1 if eos is None else int(eos), 0 if pad is None else int(pad), rows, V,
                                              embed.shape[1], mask.shape[1], _stream()), "wg_llama_pick_token")
