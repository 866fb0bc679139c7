"""What the SAM image encoder and the CLIP tower share on the host side: the cache of derived kernel operands (_Prepared, _tiled), keyed
by tensor_key, and the pre-LN transformer block both encoders stack (PreLNBlock) with its three GEMM chains: bf16, MX fp8, per-row fp8."""
import weakref

import torch

from . import ops

BF16 = torch.bfloat16


def tensor_key(t):
    """Identity of a tensor's contents as far as the host can see it: a moved, replaced, re-typed or in-place edited tensor has another key."""
    return (t.data_ptr(), t._version, t.dtype, t.device)


class _Prepared:
    """Derived (re-laid / concatenated / bf16) kernel operands, rebuilt after any parameter change."""

    def _prep_get(self, build, deps=None, slot=""):
        """deps: the tensors `build` reads (default: every parameter below this module -- pass them explicitly where the module
        tree is large, the key is recomputed on every forward).  slot: a second, independently keyed set on the same module."""
        if deps is None:
            deps = self.parameters(recurse=True)
        key = tuple(tensor_key(p) for p in deps if p is not None)
        if getattr(self, "_prep_key" + slot, None) != key:
            object.__setattr__(self, "_prep_val" + slot, build())
            object.__setattr__(self, "_prep_key" + slot, key)
        return getattr(self, "_prep_val" + slot)


def _check_bf16_gpu(t, what):
    if not t.is_cuda or t.dtype != BF16:
        raise RuntimeError("%s must be a bf16 GPU tensor for the walkgpt_amd HIP path (got %s on %s); "
                           "cast the model and inputs with .bfloat16().cuda() -- there is no CPU fallback"
                           % (what, t.dtype, t.device))


_TILED = {}   # id(weight Parameter) -> (weak reference, identity key, fragment-order copy); tensors compare element-wise, so no WeakKeyDictionary


def _tiled(weight, k_slices=1):
    """ops.tile_weight(weight), cached until the parameter's storage, version, dtype or device changes (the token-side decoder kernels and
    the skinny GEMMs stream their weight matrices in MFMA fragment order; the copy is made once per checkpoint)."""
    key = tensor_key(weight) + (k_slices,)
    wid = id(weight)
    ent = _TILED.get(wid)
    if ent is None or ent[0]() is not weight or ent[1] != key:
        with torch.no_grad():
            tiled = ops.tile_weight(weight.detach().contiguous(), k_slices)
        ent = (weakref.ref(weight, lambda _r, wid=wid: _TILED.pop(wid, None)), key, tiled)
        _TILED[wid] = ent
    return ent[2]


def _cat(tensors):
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, 0).contiguous()


class PreLNBlock(_Prepared):
    """x += proj(attention(qkv(LN1(x)))); x += fc2(act(fc1(LN2(x)))) on ops.Rows, both LayerNorms folded into the GEMM behind them.
    A concrete block supplies
      _parts()                    (norm1, norm2, q|k|v weights, q|k|v biases, proj, fc1, fc2, activation code): its LayerNorms and Linears;
                                  the q|k|v weights / biases are tuples that the cached builders concatenate (one packed parameter or three);
      _attend(qkv, ctx, mx_out)   its attention on the packed qkv rows -> a bf16 tensor, or an ops.Rows (with mx_out it may carry the MX
                                  form the proj GEMM reads; where it does not, the chain quantises).  ctx is the caller's own per-call
                                  context, handed through _block untouched."""

    gemm_dtype = "bf16"   # "fp8": qkv / proj / fc1 / fc2 on e4m3 operands (BASELINE config C5); set through WalkGPTGrounding.set_gemm_dtype

    _SLOTS = {"bf16": "", "mx": "_mx", "fp8": "_fp8"}

    # ---- the derived operands of the three chains, each keyed on exactly the tensors its builder reads --------------------------------
    @staticmethod
    def _chain_deps(chain, parts):
        n1, n2, ws, bs, proj, fc1, fc2, _ = parts
        if chain == "fp8":
            return (*ws, *bs, proj.weight, fc1.weight, fc2.weight)
        folds = (n1.weight, n1.bias, *ws, *bs, n2.weight, n2.bias, fc1.weight, fc1.bias, fc2.weight)
        return folds + (proj.weight,) if chain == "mx" else folds

    def _operands(self, chain, parts):
        return self._prep_get(getattr(self, "_build_" + chain), self._chain_deps(chain, parts), slot=self._SLOTS[chain])

    def _build_bf16(self):
        n1, n2, ws, bs, _, fc1, fc2, _ = self._parts()
        w2 = fc2.weight
        if (w2.shape[1] * 2) % 10240 == 0 and w2.is_cuda:
            # SAM ViT-H's lin2 (K = 5120): weight rows on a 10 240-byte pitch camp on a few memory channels -- the same rows 128 bytes further apart run
            # the GEMM 10 % faster (tools/bench_gemm_pitch.py, notes/r06_experiments.md section 7; K = 3072 / 4096 rows measured no difference)
            buf = torch.empty(w2.shape[0], w2.shape[1] + 64, device=w2.device, dtype=w2.dtype)
            buf[:, :w2.shape[1]].copy_(w2.detach())
            w2 = buf[:, :w2.shape[1]]
        return {"qkv": ops.fold_layernorm(n1.weight, n1.bias, _cat(ws), _cat(bs)),
                "fc1": ops.fold_layernorm(n2.weight, n2.bias, fc1.weight, fc1.bias), "fc2": w2}

    def _build_mx(self):
        n1, n2, ws, bs, proj, fc1, fc2, _ = self._parts()
        return {"qkv": ops.fold_layernorm_mx(n1.weight, n1.bias, _cat(ws), _cat(bs)), "proj": ops.mx_weight(proj.weight),
                "fc1": ops.fold_layernorm_mx(n2.weight, n2.bias, fc1.weight, fc1.bias), "fc2": ops.mx_weight(fc2.weight)}

    def _build_fp8(self):
        _, _, ws, bs, proj, fc1, fc2, _ = self._parts()
        return {"qkv": ops.quantize_weight_fp8(_cat(ws)), "bqkv": _cat(bs), "proj": ops.quantize_weight_fp8(proj.weight),
                "fc1": ops.quantize_weight_fp8(fc1.weight), "fc2": ops.quantize_weight_fp8(fc2.weight)}

    def _chain(self, parts):
        """Which chain the next forward takes: gemm_dtype, then the widths (fp8 runs as the MX chain where the persistent MX kernel takes them)."""
        if self.gemm_dtype != "fp8":
            return "bf16"
        return "mx" if ops.mx_chain_ok(parts[0].weight.shape[0], parts[5].weight.shape[0]) else "fp8"

    def prepare(self):
        """Build (or refresh) the derived operands the next forward will read, on the CURRENT stream: a caller that runs slices of a batch on side
        streams calls this before it forks, so that no slice builds them lazily on one stream while another reads them unordered."""
        parts = self._parts()
        return self._operands(self._chain(parts), parts)

    # ---- the three chains ---------------------------------------------------------------------------------------------------------------
    def _block(self, r, ctx, tail_tiles=False):
        """r: ops.Rows of the block's input rows -> the same of its output.  The parts are looked up once per call: every chain reads them,
        and so does the key of its operands."""
        parts = self._parts()
        chain = self._chain(parts)
        if chain == "bf16":
            return self._chain_bf16(r, ctx, parts, tail_tiles)
        return self._chain_mx(ops.mx_rows(r), ctx, parts) if chain == "mx" else self._chain_fp8(r, ctx, parts)

    def _chain_bf16(self, r, ctx, parts, tail_tiles):
        """tail_tiles: let the GEMMs use the tail-absorbing tiles (faster when nothing else shares the GPU, slower under stream overlap)."""
        n1, n2, _, _, proj, _, fc2, act = parts
        w = self._operands("bf16", parts)
        qkv = ops.ln_linear(r, w["qkv"], n1.eps, tail_tiles=tail_tiles)
        o = self._attend(qkv, ctx, False)
        # proj and fc2 write the residual stream that norm2 / the next block's norm1 read: they leave the rows' partial sums next
        # to them (ops.Rows) and ln_linear picks those up (no statistics pass in between)
        r = ops.linear(o, proj.weight, proj.bias, residual=r.x, tail_tiles=tail_tiles, row_partials=True)
        h = ops.ln_linear(r, w["fc1"], n2.eps, act=act, tail_tiles=tail_tiles)
        return ops.linear(h, w["fc2"], fc2.bias, residual=r.x, tail_tiles=tail_tiles, row_partials=True)

    def _chain_mx(self, r, ctx, parts):
        """The block as one MX chain on the persistent fp8 GEMM (ops.linear_mxfp8): e4m3 operands with a power-of-two scale per 32
        values on both sides; both LayerNorms folded into the GEMM behind them from the partial sums the GEMM in front left; the
        residual GEMMs (proj, fc2) leave the stream as bf16 AND as the next GEMM's e4m3 operand; the MLP's hidden layer only ever
        exists as e4m3.  SAM's attention kernels write their output as the proj GEMM's MX operand themselves at head_dim 64; at ViT-H's 80 a
        32-column block would straddle two heads, and CLIP's attention writes bf16: there the attention output keeps one quantisation pass per
        block.  Attention, the residual stream and every statistic stay bf16 / fp32."""
        n1, n2, _, _, proj, _, fc2, act = parts
        w = self._operands("mx", parts)
        qkv = ops.linear_mxfp8(r, w["qkv"], ln_eps=n1.eps)
        o = self._attend(qkv, ctx, True)
        if not isinstance(o, ops.Rows):
            o = ops.Rows(o)
        if o.mx is None:                   # (the attention kernel wrote bf16: the quantisation is a pass of its own)
            o = ops.quantize_mx_fp8(o.x)
        r = ops.linear_mxfp8(o, w["proj"], bias=proj.bias, residual=r.x, mx_out=True, row_partials=True)
        h = ops.linear_mxfp8(r, w["fc1"], act=act, ln_eps=n2.eps, mx_out=True, bf16_out=False)
        return ops.linear_mxfp8(h, w["fc2"], bias=fc2.bias, residual=r.x, mx_out=True, row_partials=True)

    def _chain_fp8(self, r, ctx, parts):
        """Widths the MX kernel does not take, with per-row activation scales: both LayerNorms fused with the per-row quantisation of their
        output."""
        n1, n2, _, _, proj, fc1, fc2, act = parts
        w = self._operands("fp8", parts)
        x = r.x
        q, s = ops.quantize_rows_fp8(x, ln=(n1.weight, n1.bias), eps=n1.eps)
        qkv = ops.linear_fp8(q, s, *w["qkv"], bias=w["bqkv"])
        q, s = ops.quantize_rows_fp8(self._attend(qkv, ctx, False))
        x = ops.linear_fp8(q, s, *w["proj"], bias=proj.bias, residual=x)
        q, s = ops.quantize_rows_fp8(x, ln=(n2.weight, n2.bias), eps=n2.eps)
        q, s = ops.quantize_rows_fp8(ops.linear_fp8(q, s, *w["fc1"], bias=fc1.bias, act=act))
        return ops.Rows(ops.linear_fp8(q, s, *w["fc2"], bias=fc2.bias, residual=x))
