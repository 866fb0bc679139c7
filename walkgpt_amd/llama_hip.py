"""The language model's generate path on the HIP kernels of csrc/llama.hip: a causal prefill through the bf16 GEMMs and a KV-cache decode
step of weight-streaming GEMVs, captured once into a HIP graph and replayed per token.  Opt-in (walkgptForCausalLM.enable_hip_llm); the
runner reads the `transformers` LlamaForCausalLM's own weight tensors -- nothing is packed or copied.

Unmerged LoRA adapters on q_proj, k_proj and / or v_proj (PEFT's lora.Linear, recognised by its attributes: peft itself is not needed) are
computed as W x + scaling * B (A x) without a further launch in the decode step: the rows of A are further weight rows of the q | k | v
GEMV (t = A xh, fp32, into a [rows, 3 r] buffer) and the rope + cache kernel adds scaling * B t to the q, k, v elements it reads anyway.
The runner reads the modules' own base_layer.weight, lora_A[name].weight and lora_B[name].weight.  A merged or disabled layer counts
as its base_layer; a model without active adapters takes the plain entry points.

Decode step, per layer: gemv (RMSNorm -> q | k | v), rope + cache write, decode attention (+ its combine), gemv (o_proj + residual), gemv (RMSNorm ->
SwiGLU), gemv (down_proj + residual); then the final RMSNorm into the hidden-state buffer, the lm_head gemv and the device-side token pick.  After
the pick a step needs nothing from the host: the host only looks at the tokens every `sync_every` steps to see whether every row has finished.

Memory kept between calls (one (rows, cap) signature only): the KV cache, 2 * layers * rows * cap * hidden * 2 bytes (a 7B model at cap 896:
0.47 GB per row), the hidden-state buffer rows * cap * hidden * 2 bytes and a few row-sized work buffers.

weights="e4m3" (W8A16, decode on half the weight bytes): the seven projections of every layer are kept a second time as OCP e4m3 bytes with
one power-of-two fp32 scale per output row (the format at include/walkgpt_hip.h; ops.llama_quantize_weight), in a store keyed by each source
tensor's (data_ptr, _version, dtype): built on first use, and an edited or replaced weight is quantised again -- that one alone -- by the
same key change that re-captures the graph.  The decode GEMVs read the bytes (wg_llama_gemv_e4m3, with adapters wg_llama_gemv_lora_e4m3); lm_head,
the embedding, the norms, the LoRA A / B, the KV cache and the attention kernels stay bf16.  The dequantised W' = q * scale is exactly a
bf16 value, so the mode is an ordinary LLaMA with the weights W': the prefill dequantises each projection into one reused bf16 scratch
buffer (sized for the largest projection) and runs the bf16 GEMMs on it, the same model the decode step runs.
Its memory cost: one byte per projection weight plus 4 bytes per output row -- 6.5 GB for a 7B model -- BESIDE the model's own bf16
tensors, which are not freed and not touched (model_forward and training go on reading them), and the scratch buffer (90 MB at 7B)."""
import math

import torch
from torch import nn

from . import ops

BF16 = torch.bfloat16
MAX_ROWS = 8


def _rope_params(config):
    p = getattr(config, "rope_parameters", None) or getattr(config, "rope_scaling", None) or {}
    theta = p.get("rope_theta", getattr(config, "rope_theta", None))
    return (10000.0 if theta is None else float(theta)), p.get("rope_type", p.get("type", "default")) or "default"


def rope_table(config, max_pos):
    """cos, sin fp32 [max_pos, 64] of the default rope type, by LlamaRotaryEmbedding's formula: inv_freq = theta^(-2i / 128) in fp32, angle = position
    * inv_freq in fp32 (the two halves of transformers' [.., 128] table are equal, so 64 columns hold all of it)."""
    theta, _ = _rope_params(config)
    inv_freq = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    freqs = torch.arange(max_pos, dtype=torch.float)[:, None] * inv_freq[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def trimmed_length(tokens, eos, max_new_tokens):
    """How many of the emitted tokens `_generate` returns: it stops after the step at which every row has emitted eos (a finished row goes on
    emitting pad), else after max_new_tokens.  tokens: int64 [rows, steps] (steps <= max_new_tokens) -> n in 1 .. max_new_tokens, or None when
    the steps seen so far do not decide it yet."""
    steps = tokens.shape[1]
    if eos is not None and steps > 0:
        hit = tokens == eos
        if bool(hit.any(1).all()):
            return int(hit.int().argmax(1).max()) + 1
    return max_new_tokens if steps >= max_new_tokens else None


LORA_TARGETS = ("q_proj", "k_proj", "v_proj")


def _is_lora(m):
    """PEFT's lora.Linear by its attributes: a Linear at base_layer, ModuleDicts lora_A / lora_B from adapter name to a Linear."""
    return isinstance(getattr(m, "base_layer", None), nn.Linear) and isinstance(getattr(m, "lora_A", None), nn.ModuleDict) \
        and isinstance(getattr(m, "lora_B", None), nn.ModuleDict)


def _active_adapters(m):
    """The adapter names the layer's own forward would apply: none when it is merged or disabled."""
    if getattr(m, "merged", False) or getattr(m, "disable_adapters", False):
        return []
    names = getattr(m, "active_adapters", None) or []
    names = [names] if isinstance(names, str) else list(names)
    return [a for a in names if a in m.lora_A and a in m.lora_B]


def _base(m):
    return m.base_layer if _is_lora(m) else m


def _adapter(m):
    """-> None for a plain (or merged / disabled) projection, else (name, A [r, in], B [out, r], scaling) of its one active adapter."""
    if not _is_lora(m):
        return None
    names = _active_adapters(m)
    if not names:
        return None
    a = names[0]
    return a, m.lora_A[a].weight, m.lora_B[a].weight, float(m.scaling[a])


class _Buffers:
    pass


WEIGHT_MODES = ("bf16", "e4m3")


def check_weight_mode(weights):
    if weights not in WEIGHT_MODES:
        raise ValueError("weights=%r: the HIP LLaMA path takes \"bf16\" or \"e4m3\"" % (weights,))
    return weights


def tensor_key(t):
    return (t.data_ptr(), t._version, t.dtype)


class WeightStore:
    """What `quantize(tensor)` gave for each source tensor, keyed by tensor_key: refresh(tensors) builds the entries whose key is new (a
    first use, an in-place edit, a replaced tensor), keeps the others as they are and drops those no tensor has any more."""

    def __init__(self, quantize):
        self._quantize = quantize
        self._items = {}
        self.builds = 0              # how many entries have been built (tests: an edit rebuilds one)

    def refresh(self, tensors):
        items = {}
        for t in tensors:
            k = tensor_key(t)
            if k in items:
                continue
            item = self._items.get(k)
            if item is None:
                item = self._quantize(t)
                self.builds += 1
            items[k] = item
        self._items = items

    def __getitem__(self, t):
        return self._items[tensor_key(t)]

    def __len__(self):
        return len(self._items)


class LlamaHipRunner:
    def __init__(self, llm, weights="bf16"):
        self.weights = check_weight_mode(weights)
        ok, why = self.supports(llm)
        if not ok:
            raise ValueError("LlamaHipRunner: " + why)
        self.llm = llm
        self._store = WeightStore(ops.llama_quantize_weight) if weights == "e4m3" else None
        self._scratch = None         # e4m3 prefill: the bf16 buffer every projection is dequantised into
        cfg = llm.config
        self.hidden, self.inter, self.heads = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
        self.eps = float(cfg.rms_norm_eps)
        self.scale = 1.0 / math.sqrt(128.0)
        self._buf = None
        self._graph = None
        self.captures = 0            # how many times a decode step has been captured (tests: a second generate replays)

    # -- what the kernels cover ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def supports(llm):
        cfg = getattr(llm, "config", None)
        if cfg is None or not hasattr(llm, "model") or not hasattr(llm, "lm_head"):
            return False, "not a LlamaForCausalLM-shaped module (config, model, lm_head)"
        heads = cfg.num_attention_heads
        hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // heads
        if hd != 128:
            return False, "head_dim %d: the attention kernels are built for 128" % hd
        if getattr(cfg, "num_key_value_heads", heads) != heads:
            return False, "grouped-query attention (num_key_value_heads %s != num_attention_heads %d) is not built" % (cfg.num_key_value_heads, heads)
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            return False, "attention / MLP bias is not built"
        if getattr(cfg, "hidden_act", "silu") != "silu":
            return False, "hidden_act %r: only silu" % (cfg.hidden_act,)
        if _rope_params(cfg)[1] != "default":
            return False, "rope scaling (%s) is not built: default rope only" % _rope_params(cfg)[1]
        if cfg.hidden_size % 128 or cfg.intermediate_size % 128 or cfg.hidden_size != heads * 128:
            return False, "hidden size %d / intermediate size %d must be multiples of 128 (hidden = heads * 128)" % (cfg.hidden_size, cfg.intermediate_size)
        tensors = [llm.get_input_embeddings().weight, llm.model.norm.weight]
        linears = [("lm_head", llm.lm_head)]
        for i, layer in enumerate(llm.model.layers):
            tensors += [layer.input_layernorm.weight, layer.post_attention_layernorm.weight]
            linears += [("layers.%d.self_attn.%s" % (i, n), getattr(layer.self_attn, n)) for n in ("q_proj", "k_proj", "v_proj", "o_proj")]
            linears += [("layers.%d.mlp.%s" % (i, n), getattr(layer.mlp, n)) for n in ("gate_proj", "up_proj", "down_proj")]
        adapters, first_rank = [], None
        for name, m in linears:
            if _is_lora(m) and type(m.base_layer) is nn.Linear:
                why = LlamaHipRunner._lora_refusal(name, m)
                if why:
                    return False, why
                ad = _adapter(m)
                if ad is not None:
                    r = ad[1].shape[0]
                    if first_rank is not None and r != first_rank[1]:
                        return False, "%s: LoRA rank %d differs from the rank %d of %s: one rank per model" % (name, r, first_rank[1], first_rank[0])
                    first_rank = first_rank or (name, r)
                    adapters += [(name, ad[1]), (name, ad[2])]
                m = m.base_layer
            if type(m) is not nn.Linear:
                return False, "%s is a %s, not a plain nn.Linear: merge the adapters first" % (name, type(m).__name__)
            if m.bias is not None:
                return False, "%s has a bias: not built" % name
            tensors.append(m.weight)
        for t in tensors:
            if t.dtype != BF16 or not t.is_cuda:
                return False, "weights must be bf16 on a GPU (found %s on %s)" % (str(t.dtype).replace("torch.", ""), t.device)
            if not t.is_contiguous():
                return False, "weights must be contiguous"
        for name, t in adapters:
            if t.dtype != BF16 or not t.is_cuda or not t.is_contiguous():
                return False, "%s: adapter weights must be contiguous bf16 on a GPU (found %s on %s)" % (name, str(t.dtype).replace("torch.", ""), t.device)
        return True, ""

    @staticmethod
    def _lora_refusal(name, m):
        """Why the LoRA layer `m` (PEFT's lora.Linear by its attributes) is not covered, or None.  Structure only: no dtype, no device."""
        names = _active_adapters(m)
        if not names:
            return None                          # merged or disabled: its own forward is base_layer's
        if name.rsplit(".", 1)[-1] not in LORA_TARGETS:
            return "LoRA on %s: only q_proj, k_proj and v_proj adapters are built; merge the others" % name
        if len(names) > 1:
            return "%s: %d active adapters (%s): one active adapter per layer is built" % (name, len(names), ", ".join(names))
        a = names[0]
        if (getattr(m, "use_dora", None) or {}).get(a, False):
            return "%s: adapter %r uses DoRA: not built" % (name, a)
        A, B = m.lora_A[a], m.lora_B[a]
        if not isinstance(A, nn.Linear) or not isinstance(B, nn.Linear):
            return "%s: lora_A / lora_B of adapter %r are not nn.Linear" % (name, a)
        if B.bias is not None or A.bias is not None:
            return "%s: lora_%s of adapter %r has a bias: not built" % (name, "B" if B.bias is not None else "A", a)
        r = A.weight.shape[0]
        if A.weight.shape != (r, m.base_layer.in_features) or B.weight.shape != (m.base_layer.out_features, r):
            return "%s: adapter %r has shapes %s / %s that do not fit the base layer" % (name, a, tuple(A.weight.shape), tuple(B.weight.shape))
        if r % 8 or not 8 <= r <= 64:
            return "%s: LoRA rank %d: the kernels take multiples of 8 up to 64" % (name, r)
        if a not in getattr(m, "scaling", {}):
            return "%s: adapter %r has no scaling" % (name, a)
        drop = getattr(m, "lora_dropout", None)
        drop = drop[a] if drop is not None and a in drop else None
        if m.training and isinstance(drop, nn.Dropout) and drop.p > 0:
            return "%s: LoRA dropout p = %g is live in training mode: call eval() first" % (name, drop.p)
        return None

    # -- weights -----------------------------------------------------------------------------------------------------------------------------
    def _layers(self):
        """Per layer the nine base weights, then the adapters: None (the plain path), or per q, k, v projection None or (name, A, B, scaling)."""
        out = []
        for layer in self.llm.model.layers:
            a, m = layer.self_attn, layer.mlp
            lora = tuple(_adapter(getattr(a, n)) for n in LORA_TARGETS)
            out.append((layer.input_layernorm.weight, _base(a.q_proj).weight, _base(a.k_proj).weight, _base(a.v_proj).weight, _base(a.o_proj).weight,
                        layer.post_attention_layernorm.weight, _base(m.gate_proj).weight, _base(m.up_proj).weight, _base(m.down_proj).weight,
                        lora if any(ad is not None for ad in lora) else None))
        return out

    def _head(self):
        return _base(self.llm.lm_head).weight

    def _rank(self):
        """The adapters' common rank (supports() has seen to it that there is one), 0 without adapters."""
        for lw in self._layers():
            for ad in lw[9] or ():
                if ad is not None:
                    return int(ad[1].shape[0])
        return 0

    def _weight_key(self):
        """What a captured decode step has baked in: data_ptr, _version and dtype of every weight, and per adapted projection the adapter's
        name, the same of its A and B, and its scaling.  A merged or disabled adapter is absent from it, so switching one changes the key."""
        key = [tensor_key(t) for t in (self.llm.model.norm.weight, self._head(), self.llm.get_input_embeddings().weight)]
        for lw in self._layers():
            key += [tensor_key(t) for t in lw[:9]]
            if lw[9] is not None:
                key.append(tuple(None if ad is None else (ad[0], tensor_key(ad[1]), tensor_key(ad[2]), ad[3]) for ad in lw[9]))
        return tuple(key)

    # -- the e4m3 store ----------------------------------------------------------------------------------------------------------------------
    def _refresh_store(self):
        """e4m3: (re)quantise the projections whose source tensor is new or has changed; called before anything reads the store."""
        if self._store is not None:
            ws = [w for lw in self._layers() for w in lw[1:5] + lw[6:9]]
            self._store.refresh(ws)
            self._scratch_numel = max(w.numel() for w in ws)

    def _gemv(self, x, ws, **kw):
        """The decode GEMV of projection weights `ws`: their bytes and scales in e4m3 mode"""
        if self._store is None:
            return ops.llama_gemv(x, ws, **kw)
        qs = [self._store[w] for w in ws]
        return ops.llama_gemv(x, [q for q, _ in qs], scales=[s for _, s in qs], **kw)

    def _linear(self, x, w, **kw):
        """The prefill GEMM of projection weight `w`: in e4m3 mode on W' = q * scale, dequantised into the scratch buffer"""
        if self._store is None:
            return ops.linear(x, w, **kw)
        if self._scratch is None or self._scratch.numel() < self._scratch_numel or self._scratch.device != w.device:
            self._scratch = torch.empty(self._scratch_numel, device=w.device, dtype=BF16)
        q, s = self._store[w]
        return ops.linear(x, ops.llama_dequantize_weight(q, s, out=self._scratch[:w.numel()].view(w.shape)), **kw)

    # -- buffers of one (rows, cap) signature ------------------------------------------------------------------------------------------------
    def _buffers(self, rows, cap, dev):
        b = self._buf
        if b is not None and (b.rows, b.cap, b.dev) == (rows, cap, dev):
            r = self._rank()
            if r and (b.t is None or b.t.shape[1] != 3 * r):
                b.t = torch.zeros(rows, 3 * r, device=dev, dtype=torch.float32)
                self._graph = None               # a captured step holds the old buffer
            return b
        self._buf = self._graph = None           # the old signature's cache and graph go first: two caches need not fit
        b = _Buffers()
        b.rows, b.cap, b.dev = rows, cap, dev
        H, I, V = self.hidden, self.inter, self._head().shape[0]
        e = lambda *s, dtype=BF16: torch.empty(*s, device=dev, dtype=dtype)
        b.kv = [(e(rows, cap, H), e(rows, cap, H)) for _ in self.llm.model.layers]
        b.hs = e(rows, cap, H)
        b.mask = torch.zeros(rows, cap, device=dev, dtype=torch.uint8)
        b.state = torch.zeros(2, device=dev, dtype=torch.int32)      # {past_len, n_new}
        b.zero = torch.zeros(1, device=dev, dtype=torch.int32)
        b.finished = torch.zeros(rows, device=dev, dtype=torch.int32)
        b.tokens = torch.zeros(rows, cap, device=dev, dtype=torch.int64)
        b.x, b.qkv, b.q, b.attn, b.act = e(rows, H), e(rows, 3 * H), e(rows, H), e(rows, H), e(rows, I)
        b.x.zero_()
        r = self._rank()
        b.t = torch.zeros(rows, 3 * r, device=dev, dtype=torch.float32) if r else None      # the adapters' down-projections of a decode step
        b.logits = e(rows, V, dtype=torch.float32)
        b.ws = ops.llama_attn_decode_workspace(rows, self.heads, dev)
        cos, sin = rope_table(self.llm.config, cap)
        b.cos, b.sin = cos.to(dev), sin.to(dev)
        self._buf = b
        return b

    # -- prefill -----------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, inputs_embeds, attention_mask, cap=None, all_logits=False):
        """-> (post-model.norm hidden states [rows, L0, H] bf16, fp32 logits [rows, V] of the last position or [rows, L0, V] of all).  Fills the KV
        cache of the (rows, cap) buffers; all_logits runs the lm_head 8 rows at a time (a checking aid, not a fast path).
        Adapters: their down-projection t = xn A^T goes through the decode GEMV with the roles swapped -- 8 rows of A as its `x`, the
        rows * L0 rows of xn as its weight, fp32 output t^T, one launch per 8 rows of A (_prefill_lora_t) -- and the rope + cache kernel
        adds the up-projection.  xn is here the bf16-rounded output of the RMSNorm kernel; the decode step's GEMV takes it unrounded."""
        rows, L0, H = inputs_embeds.shape
        if rows > MAX_ROWS:
            raise NotImplementedError("LlamaHipRunner: %d rows (the decode GEMV takes at most %d)" % (rows, MAX_ROWS))
        assert H == self.hidden and inputs_embeds.dtype == BF16 and inputs_embeds.is_cuda
        cap = (L0 + 63) // 64 * 64 if cap is None else cap
        assert cap % 64 == 0 and cap >= L0
        b = self._buffers(rows, cap, inputs_embeds.device)
        self._refresh_store()
        b.mask.zero_()
        b.mask[:, :L0] = attention_mask.to(torch.uint8)
        M, I, heads = rows * L0, self.inter, self.heads
        h = inputs_embeds.reshape(M, H).contiguous()
        qkv = torch.empty(M, 3 * H, device=h.device, dtype=BF16)
        q = torch.empty(M, H, device=h.device, dtype=BF16)
        gu = torch.empty(M, 2 * I, device=h.device, dtype=BF16)
        r = self._rank()
        t = torch.zeros(M, 3 * r, device=h.device, dtype=torch.float32) if r else None      # the adapters' down-projections, reused by every layer
        tt = torch.empty(r, M, device=h.device, dtype=torch.float32) if r else None
        for (ln1, wq, wk, wv, wo, ln2, wg, wu, wd, lora), (kc, vc) in zip(self._layers(), b.kv):
            xn = ops.rmsnorm(h, ln1, self.eps)
            for i, w in enumerate((wq, wk, wv)):
                self._linear(xn, w, out=qkv[:, i * H:(i + 1) * H])
            if lora is None:
                ops.llama_rope_cache(qkv, b.cos, b.sin, b.zero, q, kc, vc, rows, L0, heads)
            else:
                ops.llama_rope_cache(qkv, b.cos, b.sin, b.zero, q, kc, vc, rows, L0, heads, t=self._prefill_lora_t(xn, lora, t, tt),
                                     lora_b=[ad and ad[2] for ad in lora], lora_scale=[ad[3] if ad else 0.0 for ad in lora])
            att = ops.llama_attn_prefill(q, kc, vc, b.mask, b.zero, L0, heads, self.scale)
            h = self._linear(att, wo, residual=h)
            xn = ops.rmsnorm(h, ln2, self.eps)
            self._linear(xn, wg, out=gu[:, :I])
            self._linear(xn, wu, out=gu[:, I:])
            h = self._linear(ops.llama_silu_mul(gu), wd, residual=h)
        norm_w, head_w = self.llm.model.norm.weight, self._head()
        h3 = h.view(rows, L0, H)
        for r in range(rows):
            ops.rmsnorm(h3[r], norm_w, self.eps, out=b.hs[r, :L0])
        hidden = b.hs[:, :L0]
        ops.llama_gemv(h3[:, -1], [head_w], gamma=norm_w, eps=self.eps, out=b.logits, out_f32=True)
        if not all_logits:
            return hidden, b.logits
        logits = torch.empty(M, head_w.shape[0], device=h.device, dtype=torch.float32)
        for m0 in range(0, M, MAX_ROWS):
            ops.llama_gemv(h[m0:m0 + MAX_ROWS], [head_w], gamma=norm_w, eps=self.eps, out=logits[m0:m0 + MAX_ROWS], out_f32=True)
        return hidden, logits.view(rows, L0, -1)

    @staticmethod
    def _prefill_lora_t(xn, lora, t, tt):
        """Fills t [M, 3 r] fp32, column block i = xn A_i^T for the adapted ones of q, k, v (the others are not read): the GEMV kernel with
        xn [M, K] as its weight and 8 rows of A_i as its input gives 8 rows of t^T in tt [r, M]; the transposed copy into t is the only step
        outside the kernels."""
        r = tt.shape[0]
        for i, ad in enumerate(lora):
            if ad is None:
                continue
            for j in range(0, r, MAX_ROWS):
                ops.llama_gemv(ad[1][j:j + MAX_ROWS], [xn], out=tt[j:j + MAX_ROWS], out_f32=True)
            t[:, i * r:(i + 1) * r] = tt.t()
        return t

    # -- one decode step: a linear chain of launches on the current stream, no allocation, no host read ---------------------------------------
    def _decode_step(self, b, eos, pad):
        past, heads = b.state[0:1], self.heads
        for (ln1, wq, wk, wv, wo, ln2, wg, wu, wd, lora), (kc, vc) in zip(self._layers(), b.kv):
            if lora is None:
                self._gemv(b.x, [wq, wk, wv], gamma=ln1, eps=self.eps, out=b.qkv)
                ops.llama_rope_cache(b.qkv, b.cos, b.sin, past, b.q, kc, vc, b.rows, 1, heads)
            else:                                # the adapters ride in the same two launches
                self._gemv(b.x, [wq, wk, wv], gamma=ln1, eps=self.eps, out=b.qkv, lora_a=[ad and ad[1] for ad in lora], t_out=b.t)
                ops.llama_rope_cache(b.qkv, b.cos, b.sin, past, b.q, kc, vc, b.rows, 1, heads, t=b.t, lora_b=[ad and ad[2] for ad in lora],
                                     lora_scale=[ad[3] if ad else 0.0 for ad in lora])
            ops.llama_attn_decode(b.q, kc, vc, b.mask, past, heads, self.scale, workspace=b.ws, out=b.attn)
            self._gemv(b.attn, [wo], residual=b.x, out=b.x)
            self._gemv(b.x, [wg, wu], gamma=ln2, eps=self.eps, out=b.act, pair=True)
            self._gemv(b.act, [wd], residual=b.x, out=b.x)
        norm_w = self.llm.model.norm.weight
        ops.rmsnorm(b.x, norm_w, self.eps, out=b.hs, slot=past)           # the hidden state of the token at position past_len
        ops.llama_gemv(b.x, [self._head()], gamma=norm_w, eps=self.eps, out=b.logits, out_f32=True)
        self._pick(b, eos, pad)

    def _pick(self, b, eos, pad):
        ops.llama_pick_token(b.logits, self.llm.get_input_embeddings().weight, b.x, b.tokens, b.finished, b.mask, b.state, eos, pad)

    def _captured_step(self, b, eos, pad):
        """The decode step of these buffers as a HIP graph, captured on first use and again whenever a weight it reads has moved or changed
        (the key carries data_ptr, _version and dtype of every one).  Warm-up and capture run on a stream of the graph's own; they advance
        the device state, so this is called BEFORE the prefill that sets it."""
        key = (eos, pad, self._weight_key())
        if self._graph is not None and self._graph[1] == key:
            return self._graph[0]
        self._graph = None
        b.state.zero_()
        cap_stream = torch.cuda.Stream()
        cap_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap_stream):
            for _ in range(2):
                self._decode_step(b, eos, pad)
        torch.cuda.current_stream().wait_stream(cap_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap_stream):
            self._decode_step(b, eos, pad)
        self._graph = (g, key, cap_stream)
        self.captures += 1
        return g

    # -- generate ----------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, inputs_embeds, attention_mask, max_new_tokens, eos=None, pad=None, graph=True, sync_every=8):
        """walkgptForCausalLM._generate's contract: -> (new token ids [rows, n] int64, last-layer (post-norm) hidden states of the prompt and of
        every generated token that was fed back, [rows, L0 + n - 1, H]).  Greedy; rows that have emitted eos go on emitting pad; n ends at the
        step at which every row has finished, whatever sync_every is."""
        rows, L0, H = inputs_embeds.shape
        if rows > MAX_ROWS:
            raise NotImplementedError("LlamaHipRunner: %d rows (the decode GEMV takes at most %d)" % (rows, MAX_ROWS))
        assert max_new_tokens >= 1 and sync_every >= 1
        pad = eos if pad is None else pad
        cap = (L0 + max_new_tokens + 63) // 64 * 64
        b = self._buffers(rows, cap, inputs_embeds.device)
        self._refresh_store()                      # before the capture: a captured step holds the store's buffers
        g = self._captured_step(b, eos, pad) if graph else None
        self.prefill(inputs_embeds, attention_mask, cap=cap)
        b.finished.zero_()
        b.state.zero_()
        b.state[0:1].fill_(L0 - 1)                 # the pick works from the position of the token whose logits it reads
        self._pick(b, eos, pad)
        done, n = 1, None
        while n is None:
            n = trimmed_length(b.tokens[:, :done].cpu(), eos, max_new_tokens)
            if n is not None:
                break
            for _ in range(min(sync_every, max_new_tokens - done)):
                if g is not None:
                    g.replay()
                else:
                    self._decode_step(b, eos, pad)
                done += 1
        return b.tokens[:, :n].clone(), b.hs[:, :L0 + n - 1].clone()
