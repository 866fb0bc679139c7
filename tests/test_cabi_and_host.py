"""CPU-side checks (no GPU): the C-ABI library loads and exports exactly what include/walkgpt_hip.h declares, the
host modules keep the reference's checkpoint ABI, weight re-layouts are the right permutations, the synthetic
generator is deterministic, and the product path refuses to run without the GPU (no fallback)."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "walkgpt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wg_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from walkgpt_amd import _lib
    h = _lib.lib()
    declared = _header_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(h, name), "libwalkgpt_hip.so does not export %s" % name
    assert sorted(_lib.exported_symbols()) == declared, "ctypes table and header disagree"
    assert h.wg_version() >= 100
    # error plumbing works without a GPU: bad arguments are rejected before any HIP call
    rc = h.wg_layernorm_rows(None, 0, None, None, None, 0, 1, 8, 1e-5, 0, None)
    assert rc < 0 and b"layernorm" in h.wg_last_error()
    rc = h.wg_gemm_bias_act_bf16(None, 0, None, 0, None, None, 0, 0, None, 0, 1, 1, 1, 0, 0, 0, None)
    assert rc < 0


def test_state_dict_abi_matches_reference_fixture():
    from walkgpt_amd.segment_anything import build_sam_vit_b
    from walkgpt_amd.utils_walkgpt import CalibratedTextProjector, MultiScaleQFormerProjector
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_shapes.json")))
    with torch.device("meta"):
        got = {
            "sam_vit_b": build_sam_vit_b().state_dict(),
            "msqp_4096": MultiScaleQFormerProjector(256, 4096, target_square_side=6).state_dict(),
            "ctp_4096": CalibratedTextProjector(4096, 256).state_dict(),
        }
    for name, sd in got.items():
        assert {k: list(v.shape) for k, v in sd.items()} == fix[name], name


def test_clip_tower_uses_hf_parameter_names():
    from types import SimpleNamespace
    from tests.golden import cases
    from walkgpt_amd.clip_encoder import CLIPVisionTower
    c = cases.CLIPS["tiny"]
    cfg = dict(hidden_size=c["dim"], intermediate_size=4 * c["dim"], num_hidden_layers=c["layers"],
               num_attention_heads=c["heads"], image_size=c["img"], patch_size=14, layer_norm_eps=1e-5)
    args = SimpleNamespace(mm_vision_select_layer=-2, pad_train_clip_images=True, resize_vision_tower=True,
                           resize_vision_tower_size=c["img"])
    tower = CLIPVisionTower("synthetic", args, config=cfg)
    sd = tower.vision_tower.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == cases.clip_weight_shapes(c)
    # transformers<=4.31 checkpoints carry a persistent position_ids buffer: accepted and ignored
    w = dict(cases.clip_weights(c))
    w["vision_model.embeddings.position_ids"] = torch.arange(65)[None]
    tower.vision_tower.load_state_dict(w, strict=True)


def test_weight_relayouts_are_the_right_permutations():
    """The prepared GEMM operands reproduce conv / conv-transpose arithmetic (checked with torch on the CPU)."""
    import torch.nn.functional as F
    from walkgpt_amd.segment_anything import modeling as M
    g = torch.Generator().manual_seed(0)
    # neck 3x3: [O,C,3,3] -> [O,(ky,kx,c)] against rows built in (ky,kx,c) order
    x = torch.randn(1, 5, 6, 8, generator=g)  # B,H,W,C
    w = torch.randn(4, 8, 3, 3, generator=g)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, 4)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    rows = torch.stack([xp[0, y + ky, xx + kx] for y in range(5) for xx in range(6) for ky in range(3) for kx in range(3)]).reshape(30, 72)
    wr = w.permute(0, 2, 3, 1).reshape(4, -1)
    assert torch.allclose(rows @ wr.t(), ref, atol=1e-5)
    # ConvTranspose2d(k2,s2): [Cin,Cout,2,2] -> [(dy,dx,Cout),Cin]; output pixel (2y+dy, 2x+dx)
    dec = M.MaskDecoder(transformer_dim=16, transformer=M.TwoWayTransformer(depth=1, embedding_dim=16, num_heads=2, mlp_dim=32))
    t = torch.randn(1, 16, 3, 3, generator=g)
    c1 = dec.output_upscaling[0]
    ref = F.conv_transpose2d(t, c1.weight, c1.bias, stride=2)  # [1,4,6,6]
    up1_w = M.MaskDecoder._convt_as_gemm(c1.weight)             # (the GPU path then puts this matrix in MFMA fragment order: test_tile_weight_layout)
    out = t.permute(0, 2, 3, 1).reshape(9, 16) @ up1_w.t() + c1.bias.repeat(4)  # rows (y,x), cols (dy,dx,co); the bias repeats per sub-pixel
    out = out.reshape(3, 3, 2, 2, 4).permute(4, 0, 2, 1, 3).reshape(4, 6, 6)
    assert torch.allclose(out, ref[0], atol=1e-5)


def test_synth_is_deterministic_and_scaled():
    from walkgpt_amd import synth
    a = synth.param(7, "image_encoder.blocks.0.attn.qkv.weight", (12, 8))
    b = synth.param(7, "image_encoder.blocks.0.attn.qkv.weight", (12, 8))
    assert np.array_equal(a, b) and a.dtype == np.float32
    assert not np.array_equal(a, synth.param(8, "image_encoder.blocks.0.attn.qkv.weight", (12, 8)))
    assert not np.array_equal(a, synth.param(7, "image_encoder.blocks.1.attn.qkv.weight", (12, 8)))
    big = synth.normal(1, "x", (200000,))
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01
    # frozen values: a change of the generator would silently invalidate every golden vector
    frozen = [0.6657984256744385, -1.1600568294525146, -1.258841872215271, 1.5264594554901123]
    assert np.allclose(synth.normal(3, "probe", (4,)), np.array(frozen, np.float32), atol=1e-6)
    assert abs(synth.param(1, "norm1.weight", (1000,)).mean() - 1) < 0.02
    assert synth.param(1, "blocks.0.attn.rel_pos_h", (27, 64)).std() > 0.05


def test_product_path_has_no_cpu_fallback():
    from walkgpt_amd import _lib, ops
    from walkgpt_amd.segment_anything import modeling as M
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.WalkgptHipError):
        ops.linear(x, x)
    with pytest.raises(_lib.WalkgptHipError):
        ops.layernorm(x, x[0], x[0], 1e-5)
    enc = M.ImageEncoderViT(img_size=64, embed_dim=64, depth=1, num_heads=1, use_rel_pos=True, window_size=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(1, 3, 64, 64))
    # nothing under walkgpt_amd/ imports the oracle
    pkg = os.path.join(ROOT, "walkgpt_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from walkgpt_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.WalkgptHipError, match="not built"):
        _lib.lib()


def test_clip_tower_resizes_a_stock_position_table_on_load():
    """clip_encoder.py:38-55: the stock checkpoint carries the 577-row (24x24 + class) table of 336 px; the tower runs at 448 px
    (32x32 + class).  load_state_dict must take the stock table and resize it the reference's way (quirk included: rows [:-1] are
    the grid, the last row is carried over), as pinned by tests/golden/clipwrap_*.npz."""
    import numpy as np
    import torch
    from types import SimpleNamespace
    from tests.golden import cases
    from walkgpt_amd.clip_encoder import CLIPVisionTower
    c = cases.CLIPWRAPS["w56"]
    gold = cases.load("clipwrap_w56")
    cfg = dict(hidden_size=c["dim"], intermediate_size=4 * c["dim"], num_hidden_layers=1, num_attention_heads=1,
               image_size=c["old_side"] * 14, patch_size=14, layer_norm_eps=1e-5)
    args = SimpleNamespace(mm_vision_select_layer=-1, resize_vision_tower=True, resize_vision_tower_size=c["new_side"] * 14)
    tower = CLIPVisionTower("synthetic", args, config=cfg)
    sd = tower.vision_tower.state_dict()
    assert sd["vision_model.embeddings.position_embedding.weight"].shape[0] == c["new_side"] ** 2 + 1
    sd["vision_model.embeddings.position_embedding.weight"] = cases.clipwrap_table(c)          # the stock-size table
    tower.vision_tower.load_state_dict(sd, strict=True)
    got = tower.vision_tower.vision_model.embeddings.position_embedding.weight.detach().numpy()
    assert np.allclose(got, gold["table"], atol=1e-6)


# The GEMM queries, one row per shape: (M, N, K, lda, ldw, ldc, ldr) -> what wg_gemm_pick_tile, wg_gemm_pick_tile_ex (allow_tail 0 / 1),
# wg_gemm_pick_tile_mnk (allow_tail 0 / 1), wg_gemm_ln_supported, wg_gemm_row_partials_supported, wg_gemm_skinny_ln_supported and
# ops.gemm_tile_for (tail_tiles False / True) return.  Kernel ids: 1 = 128x128 tiles, 3 = row-wave, 5 = skinny, 11 = persistent 128x128,
# 12 = 128x128 with the M % 128 <= 16 leftover rows in the last row tile, 16 = persistent 256x256.
# Eleventh column: the route the launcher really takes (wg_gemm_route_of, fed ops.gemm_tile_for's answer as ops.linear feeds it) for a bf16
# output and 16-byte aligned operands, a residual where ldr != 0: the kernel id after the fallbacks (14 = one-tile 256x256 ping-pong, where 16
# cannot take the operands), + _S where that kernel runs the staged epilogue.
_E = 1 << 20
_S = 64
_GEMM_QUERIES = [
    # M <= 16: the skinny kernel when N % 16 == 0, and only at K % 128 == 0 (K = 192 takes the 128x128 tiles)
    ((8, 256, 256, 256, 256, 256, 0), (5, 5, 5, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((8, 256, 192, 192, 192, 256, 0), (5, 5, 5, 1, 1, 0, 0, 0, 1, 1, 1 + _S)),
    ((16, 4096, 4096, 4096, 4096, 4096, 0), (5, 5, 5, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((8, 100, 256, 256, 256, 100, 0), (1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1)),
    ((1, 16, 128, 128, 128, 16, 0), (5, 5, 5, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((0, 256, 256, 256, 256, 256, 0), (5, 5, 5, 5, 5, 0, 0, 0, 5, 5, 5)),
    ((8, 256, 256, 260, 256, 256, 0), (5, 5, 5, 5, 5, 0, 0, 0, 3, 3, 3)),
    ((8, 256, 256, 256, 256, 258, 0), (5, 5, 5, 5, 5, 0, 0, 0, 3, 3, 3)),
    # 17 <= M <= 128: 128x128 tiles, or the skinny kernel where its cost model says it wins
    ((17, 1024, 1024, 1024, 1024, 1024, 0), (1, 1, 1, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((32, 4096, 4096, 4096, 4096, 4096, 0), (1, 1, 1, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((96, 1024, 1024, 1024, 1024, 1024, 0), (1, 1, 1, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((128, 256, 5120, 5120, 5120, 256, 0), (1, 1, 1, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((64, 256, 192, 192, 192, 256, 0), (1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1 + _S)),
    ((100, 4096, 4096, 4104, 4096, 4096, 4096), (1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1 + _S)),
    ((128, 8192, 256, 256, 256, 8192, 0), (1, 1, 1, 5, 5, 0, 0, 1, 5, 5, 5)),
    ((128, 16384, 256, 256, 256, 16384, 0), (1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1 + _S)),
    ((129, 256, 256, 256, 256, 256, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    # M = 8 * 1025 and other M % 128 in 1..16: the tail kernel (12) only with allow_tail, N % 8 == 0, and when it fills the chip
    ((8200, 1024, 1024, 1024, 1024, 1024, 0), (16, 16, 12, 16, 12, 1, 1, 0, 16, 12, 16 + _S)),
    ((8200, 3072, 1024, 1024, 1024, 3072, 0), (16, 16, 12, 16, 12, 1, 0, 0, 16, 12, 16 + _S)),
    ((8200, 4096, 1024, 1024, 1024, 4096, 4096), (16, 16, 12, 16, 12, 1, 0, 0, 16, 12, 16 + _S)),
    ((8200, 1028, 1024, 1024, 1024, 1028, 0), (16, 16, 16, 16, 16, 0, 0, 0, 16, 16, 14)),
    ((2050, 1024, 1024, 1024, 1024, 1024, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((4112, 768, 768, 768, 768, 768, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((4113, 768, 768, 768, 768, 768, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    # N = 128 / 384 / < 256: 128x128 persistent tiles; N >= 256: 256x256 unless too few big tiles (or, with allow_tail, worse rounds)
    ((4096, 128, 256, 256, 256, 128, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((4096, 384, 768, 768, 768, 384, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((4096, 192, 256, 256, 256, 192, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((4096, 64, 64, 64, 64, 64, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((1024, 1024, 1024, 1024, 1024, 1024, 0), (11, 11, 11, 11, 11, 0, 0, 0, 11, 11, 11 + _S)),
    ((32768, 768, 768, 768, 768, 768, 768), (16, 16, 11, 16, 11, 1, 1, 0, 16, 11, 16 + _S)),
    ((32768, 2304, 768, 768, 768, 2304, 0), (16, 16, 16, 16, 16, 1, 0, 0, 16, 16, 16 + _S)),
    ((32768, 1280, 5120, 5120, 5120, 1280, 1280), (16, 16, 16, 16, 16, 1, 1, 0, 16, 16, 16 + _S)),
    ((32768, 1536, 768, 768, 768, 1536, 0), (16, 16, 16, 16, 16, 1, 0, 0, 16, 16, 16 + _S)),
    ((32768, 1152, 768, 768, 768, 1152, 0), (16, 16, 16, 16, 16, 1, 0, 0, 16, 16, 16 + _S)),
    ((16384, 1536, 768, 768, 768, 1536, 0), (16, 16, 11, 16, 11, 1, 0, 0, 16, 11, 16 + _S)),
    # padded and odd leading dimensions, K off the MFMA path's K % 64 rule
    ((4096, 1024, 1024, 1028, 1024, 1024, 0), (16, 16, 11, 16, 11, 0, 0, 0, 3, 3, 3)),
    ((4096, 1024, 1024, 1024, 1030, 1024, 0), (16, 16, 11, 16, 11, 0, 0, 0, 3, 3, 3)),
    ((4096, 1024, 1024, 1024, 1024, 1028, 0), (16, 16, 11, 16, 11, 0, 0, 0, 16, 11, 14)),
    ((4096, 1024, 1024, 1024, 1024, 1030, 0), (16, 16, 11, 16, 11, 0, 0, 0, 3, 3, 3)),
    ((4096, 1024, 1024, 1024, 1024, 1024, 1026), (16, 16, 11, 16, 11, 1, 1, 0, 3, 3, 3)),
    ((4096, 1024, 1000, 1000, 1000, 1024, 0), (16, 16, 11, 16, 11, 0, 0, 0, 3, 3, 3)),
    ((4096, 1024, 1024, 1536, 1152, 1280, 1032), (16, 16, 11, 16, 11, 1, 1, 0, 16, 11, 16 + _S)),
    # the persistent kernel's 4 GiB operand bound ((M + 256) * lda, (N + 256) * ldw below 2^31 elements) and C's 2 GiB extent
    ((_E - 257, 1024, 2048, 2048, 2048, 1024, 0), (16, 16, 16, 16, 16, 1, 1, 0, 16, 16, 16 + _S)),
    ((_E - 256, 1024, 2048, 2048, 2048, 1024, 0), (16, 16, 16, 16, 16, 0, 0, 0, 16, 16, 14 + _S)),
    ((1000, _E - 264, 2048, 2048, 2048, _E - 264, 0), (16, 16, 16, 16, 16, 1, 0, 0, 16, 16, 16 + _S)),
    ((1000, _E - 256, 2048, 2048, 2048, _E - 256, 0), (16, 16, 16, 16, 16, 0, 0, 0, 16, 16, 14 + _S)),
    ((32768, 1024, 1024, 1024, 1024, 32768, 0), (16, 16, 16, 16, 16, 1, 1, 0, 16, 16, 16 + _S)),
    ((32768, 1024, 1024, 1024, 1024, 40960, 0), (16, 16, 16, 16, 16, 0, 0, 0, 16, 16, 14)),
]


def _gemm_query_mismatches(columns):
    from walkgpt_amd import _lib, ops
    L = _lib.lib()
    bad = []
    for (M, N, K, lda, ldw, ldc, ldr), want in _GEMM_QUERIES:
        got = (L.wg_gemm_pick_tile(M, N), L.wg_gemm_pick_tile_ex(M, N, 0), L.wg_gemm_pick_tile_ex(M, N, 1),
               L.wg_gemm_pick_tile_mnk(M, N, K, 0), L.wg_gemm_pick_tile_mnk(M, N, K, 1),
               L.wg_gemm_ln_supported(M, N, K, lda, ldw, ldc), L.wg_gemm_row_partials_supported(M, N, K, lda, ldw, ldc),
               L.wg_gemm_skinny_ln_supported(M, N, K, lda, ldw, ldc),
               ops.gemm_tile_for(M, N, K, lda, ldw, ldc, ldr), ops.gemm_tile_for(M, N, K, lda, ldw, ldc, ldr, True),
               L.wg_gemm_route_of(M, N, K, lda, ldw, ldc, ldr, 1 if ldr else 0, 0, 0, 0, ops.gemm_tile_for(M, N, K, lda, ldw, ldc, ldr)))
        if [got[i] for i in columns] != [want[i] for i in columns]:
            bad.append(((M, N, K, lda, ldw, ldc, ldr), [want[i] for i in columns], [got[i] for i in columns]))
    return bad


def test_tile_selector_sees_k():
    """The kernel id host-side accounting reports is the one the library launches: M <= 16 rows take the skinny kernel (5) only when
    K % 128 == 0; K = 192 passes the MFMA path's K % 64 rule and runs on the 128x128 tiles (1).  Pinned over _GEMM_QUERIES for
    wg_gemm_pick_tile, _ex, _mnk and ops.gemm_tile_for."""
    assert _gemm_query_mismatches([0, 1, 2, 3, 4, 8, 9]) == []


# wg_gemm_route_of beyond the bf16 / aligned column: (M, N, K, lda, ldw, ldc, ldr, has_residual, res_row_mod, out_f32, align_bits, tile_hint) -> route.
# align_bits: low address bits of A | W << 4 | C << 8 | bias << 12 | R << 16.
_GEMM_ROUTES = [
    # an fp32 output fails the staged epilogue: 16 -> 14, 11 / 12 -> 1, all unstaged; 1, 2, 14 keep their kernel
    ((8200, 1024, 1024, 1024, 1024, 1024, 0, 0, 0, 1, 0, 16), 14),
    ((8200, 1024, 1024, 1024, 1024, 1024, 0, 0, 0, 1, 0, 0), 14),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 1, 0, 16), 14),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 1, 0, 11), 1),
    ((4096, 128, 256, 256, 256, 128, 0, 0, 0, 1, 0, 0), 1),
    ((8200, 1024, 1024, 1024, 1024, 1024, 0, 0, 0, 1, 0, 12), 1),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 1, 0, 1), 1),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 1, 0, 2), 2),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 1, 0, 14), 14),
    # the same calls with a bf16 output: the kernel asked for, staged
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 16), 16 + _S),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 11), 11 + _S),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 1), 1 + _S),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 2), 2 + _S),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 14), 14 + _S),
    ((8200, 1024, 1024, 1024, 1024, 1024, 0, 0, 0, 0, 0, 12), 12 + _S),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 12), 1 + _S),                  # 300 % 128 = 44 leftover rows: not the tail kernel's
    # alignment: an 8-byte aligned bias keeps 16 out (14, still staged); an 8-byte aligned residual or ldr % 8 != 0 unstages; 4-byte alignment of A,
    # W or C, or 2-byte alignment of bias or R, leaves the MFMA path
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 8 << 12, 16), 14 + _S),
    ((300, 272, 128, 128, 128, 272, 272, 1, 0, 0, 8 << 16, 16), 14),
    ((300, 272, 128, 128, 128, 272, 272, 1, 0, 0, 8 << 16, 11), 1),
    ((300, 272, 128, 128, 128, 272, 276, 1, 0, 0, 0, 16), 14),
    ((300, 272, 128, 128, 128, 272, 272, 1, 0, 0, 0, 16), 16 + _S),
    ((300, 272, 128, 128, 128, 272, 272, 0, 0, 0, 8 << 16, 16), 16 + _S),         # no residual: its bits are not looked at
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 8, 16), 3),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 8 << 4, 16), 3),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 8 << 8, 16), 3),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 4 << 12, 16), 3),
    ((300, 272, 128, 128, 128, 272, 272, 1, 0, 0, 4 << 16, 16), 3),
    # N % 8 != 0 unstages; a residual table (res_row_mod) is measured by the rows that are read: 2^20 output rows of a 1024-column residual are
    # 2 GiB, too far for the staged epilogue's 32-bit offsets, 4096 table rows are not
    ((300, 276, 128, 128, 128, 276, 0, 0, 0, 0, 0, 16), 14),
    ((_E - 512, 1024, 64, 64, 64, 1024, 1024, 1, 0, 0, 0, 16), 16 + _S),
    ((_E, 1024, 64, 64, 64, 1024, 1024, 1, 4096, 0, 0, 16), 14),                  # (C itself is 2 GiB here)
    ((_E - 512, 1024, 64, 64, 64, 1024, 2048, 1, 0, 0, 0, 16), 14),
    ((_E - 512, 1024, 64, 64, 64, 1024, 2048, 1, 4096, 0, 0, 16), 16 + _S),
    # hints: 3 is honoured, 5 only for skinny shapes, an unknown one means the 128x128 tiles
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 3), 3),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 5), 1 + _S),
    ((16, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 5), 5),
    ((300, 272, 128, 128, 128, 272, 0, 0, 0, 0, 0, 7), 1 + _S),
]


def test_gemm_route_query_is_the_launchers_decision():
    """wg_gemm_route_of answers with the kernel wg_gemm_bias_act_bf16 launches (the launcher calls the same wg_gemm_decide) and whether it runs
    the staged epilogue.  The eleventh column of _GEMM_QUERIES pins it for bf16 outputs -- the row with ldc = 1028 runs 14 where
    ops.gemm_tile_for says 16 --, _GEMM_ROUTES the fallbacks an fp32 output, alignment, N % 8 and the 2 GiB extents cause."""
    from walkgpt_amd import _lib
    assert _gemm_query_mismatches([10]) == []
    L = _lib.lib()
    bad = [(args, want, L.wg_gemm_route_of(*args)) for args, want in _GEMM_ROUTES if L.wg_gemm_route_of(*args) != want]
    assert bad == []
    assert L.wg_version() == 300            # the query only adds a symbol


@pytest.mark.parametrize("name", ["w56", "w448"])
def test_loaded_position_table_is_resized_once_in_fp32(name):
    """A checkpoint that still carries the stock position table is resized on its way into the tower with the reference's arithmetic
    (clip_encoder.py:38-55: rows [:-1] taken as the grid, last row carried over, fp32 bilinear, ONE cast) -- the same table whatever
    device the tensor sits on, equal to what the reference's own load_model produced (tests/golden/clipwrap_*.npz)."""
    from types import SimpleNamespace
    from tests.golden import cases
    from walkgpt_amd.clip_encoder import CLIPVisionTower
    c = cases.CLIPWRAPS[name]
    gold = cases.load("clipwrap_" + name)
    cfg = dict(hidden_size=c["dim"], intermediate_size=16, num_hidden_layers=1, num_attention_heads=1, image_size=c["old_side"] * 14,
               patch_size=14, layer_norm_eps=1e-5)
    args = SimpleNamespace(mm_vision_select_layer=-1, pad_train_clip_images=True, resize_vision_tower=True,
                           resize_vision_tower_size=c["new_side"] * 14)
    tower = CLIPVisionTower("synthetic", args, config=cfg)
    sd = {k: v.clone() for k, v in tower.vision_tower.state_dict().items()}
    sd["vision_model.embeddings.position_embedding.weight"] = cases.clipwrap_table(c)          # the stock-size table
    tower.vision_tower.load_state_dict(sd, strict=True)
    got = tower.vision_tower.vision_model.embeddings.position_embedding.weight
    assert got.shape == (c["new_side"] ** 2 + 1, c["dim"]) and np.array_equal(got.detach().numpy(), gold["table"])


def test_mx_scale_plane_layout_host_side():
    """Host-side helpers of the fp8 MX chain (no GPU): the row permutation inside a scale plane is a bijection of every 128- / 64-row group
    that puts rows r, r + 16, .. next to each other (the 8 / 4 MFMA fragments of a lane); the pitch covers whole 256-row tiles; dequantisation
    applies 2^(byte - 127) per (row, 32 columns)."""
    import torch
    from walkgpt_amd import ops
    for group in (128, 64):
        M = 3 * group + 37
        idx = ops.mx_scale_index(M, group=group)
        assert idx.shape == (M,) and len(set(idx.tolist())) == M
        full = ops.mx_scale_index(4 * group, group=group)
        assert sorted(full.tolist()) == list(range(4 * group))                      # a permutation of every whole group
        per = group // 16
        for r in (0, 5, group + 3):
            assert [int(full[r + 16 * k]) for k in range(per)] == list(range(int(full[r]), int(full[r]) + per))
    assert ops.mx_pitch(1) == 256 and ops.mx_pitch(256) == 256 and ops.mx_pitch(257) == 512
    assert ops.mx_chain_ok(1280, 5120) and ops.mx_chain_ok(768, 3072) and not ops.mx_chain_ok(192, 768) and not ops.mx_chain_ok(1536, 6144)
    # dequantisation on a hand-built operand
    M, K = 130, 64
    q = torch.tensor([0x38], dtype=torch.uint8).repeat(M, K)                           # e4m3 0x38 = 1.0
    mx = torch.full((K // 32, ops.mx_pitch(M)), 127, dtype=torch.uint8)
    mx[1, ops.mx_scale_index(M)[129]] = 130                                             # row 129, columns 32..63: x 8
    d = ops.mx_dequantize(q, mx)
    assert d.shape == (M, K) and float(d[129, 40]) == 8.0 and float(d[129, 3]) == 1.0 and float(d[0, 40]) == 1.0


@pytest.mark.parametrize("source", ["walkgpt_amd/csrc/attn_pipe.hip"])
def test_hand_placed_streams_have_no_unpadded_mfma_operand(source):
    """attn_pipe.hip places the instructions of its loop as `asm volatile` statements; hipcc's hazard recogniser cannot see
    that a statement is an MFMA, so neither a vector instruction the COMPILER emits directly in front of one that reads its result, nor
    compiler code reading an asm MFMA's result behind it, gets wait states (found the hard way: stale operands, wrong rows that came and went
    with the register allocation).  The lint compiles the file with the product build's flags and scans the ISA for both patterns."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_asm_hazards.py"), os.path.join(ROOT, *source.split("/"))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


_ATTN_KERNELS = (   # every kernel attn.hip and attn_window_unit.hip instantiate: <head_dim, S, waves, key bias> / <head_dim, S, waves>
    ["_Z14wg_attn_kernelILi%dELi%dELi%dELb%dEEv8AttnArgs" % k for k in
     [(hd, 0, nw, kb) for hd, nws in ((16, (1,)), (32, (1, 4, 8)), (64, (1, 3, 4, 8)), (128, (1, 4, 8))) for nw in nws for kb in (0, 1)]
     + [(64, 64, 8, 0), (80, 64, 8, 0)]]
    + ["_Z21wg_attn_window_kernelILi%dELi%dELi%dEEv8AttnArgsi" % k for k in [(64, 14, 4), (64, 32, 8), (32, 14, 7), (32, 28, 5), (80, 14, 7)]]
    + ["_Z26wg_attn_window_unit_kernelILi64ELi14ELi7EEv8AttnArgsi"])


def test_attention_kernels_are_the_recorded_set_and_do_not_spill():
    """tools/isa_fingerprint.py on the two attention sources: exactly the 29 + 1 kernels the routers reach are compiled (plain and global
    wg_attn_kernel, the five windows, the unit kernel -- a template argument nobody launches would show up here), and none of them has a
    private segment, i.e. no register spills to scratch (several sit at 250+ VGPRs)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py")]
                       + [os.path.join(ROOT, "walkgpt_amd", "csrc", f) for f in ("attn.hip", "attn_window_unit.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(_ATTN_KERNELS) == 30 and sorted(row[0] for row in rows) == sorted(_ATTN_KERNELS)
    for row in rows:
        assert re.fullmatch(r"[0-9a-f]{16}", row[1]) and [f.split("=")[0] for f in row[2:]] == ["vgpr", "agpr", "sgpr", "lds", "private"], row
        assert row[-1] == "private=0", "%s spills: %s" % (row[0], " ".join(row[2:]))


def test_environment_and_macros_choose_no_code_path():
    """What the library and the host path compute depends on their arguments alone: no environment variable picks a kernel, tile order or
    fusion, and the only compile-time switches left are the diagnostic stamp builds.  The build may read HIPCC / WG_EXTRA_HIPCC_FLAGS and
    the loader WG_LIB (which compiler, which library file), nothing else."""
    pkg = os.path.join(ROOT, "walkgpt_amd")
    csrc = os.path.join(pkg, "csrc")
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h")):
            continue
        txt = open(os.path.join(csrc, name)).read()
        assert "getenv(" not in txt, "csrc/%s reads the environment" % name
        for cond in re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", txt, flags=re.M):
            macros = set(re.findall(r"\bWG_[A-Z0-9_]+", cond.split("//")[0]))
            assert macros <= {"WG_GEMM_STAMP", "WG_ATTN_STAMP"}, "csrc/%s: #if on %s" % (name, sorted(macros))
    allowed = {"_build.py": {"HIPCC", "WG_EXTRA_HIPCC_FLAGS"}, "_lib.py": {"WG_LIB"}}
    for dirpath, _, files in os.walk(pkg):
        for name in files:
            if not name.endswith(".py"):
                continue
            txt = open(os.path.join(dirpath, name)).read()
            rel = os.path.relpath(os.path.join(dirpath, name), pkg)
            if rel in allowed:
                assert set(re.findall(r"os\.environ\.get\(\"(\w+)\"", txt)) <= allowed[rel]
                assert txt.count("os.environ") == len(re.findall(r"os\.environ\.get\(\"\w+\"", txt)), rel
            else:
                assert "os.environ" not in txt and "getenv(" not in txt, "walkgpt_amd/%s reads the environment" % rel


def test_epilogue_gelu_fit_is_within_its_stated_error():
    """csrc/wg_common.h wg_act2e<WG_ACT_GELU_ERF>: the coefficients in the source are the minimax fit tools/fit_gelu.py prints, and the formula as the
    kernel evaluates it (fp32, exp2 form, x^2 clamped to 49) stays within 2.6e-5 of x Phi(x) on the whole line -- the figure the header, DESIGN.md and
    INTEGRATION.md quote (common.py:13-26 / image_encoder.py:30 use nn.GELU's erf form)."""
    from scipy.special import erf
    txt = open(os.path.join(ROOT, "walkgpt_amd", "csrc", "wg_common.h")).read()
    body = txt[txt.index("wg_act2e(f32x2 x)"):]
    body = body[:body.index("} else {")]
    c2 = float(re.search(r"x2 \* ([0-9.eE+-]+)f - ([0-9.eE+-]+)f", body).group(1))
    c1 = -float(re.search(r"x2 \* ([0-9.eE+-]+)f - ([0-9.eE+-]+)f", body).group(2))
    c0 = -float(re.search(r"p \* x2 - ([0-9.eE+-]+)f", body).group(1))
    clamp = float(re.search(r"fminf\(x2\.x, ([0-9.]+)f\)", body).group(1))
    x = np.linspace(-14, 14, 560001).astype(np.float32)
    x2 = np.minimum(x * x, np.float32(clamp))
    with np.errstate(over="ignore"):
        y = x / (np.float32(1) + np.exp2(x * (np.float32(c0) + x2 * (np.float32(c1) + x2 * np.float32(c2)))))
    ref = x.astype(np.float64) * 0.5 * (1 + erf(x.astype(np.float64) / np.sqrt(2)))
    assert np.isfinite(y).all() and float(np.max(np.abs(y - ref))) <= 2.6e-5
    # ... and they are the fit's: (a, b, c) * -log2(e) with the tanh form's well-known a, b as a sanity anchor (a = 1.5958 -> 1.5950, b = 0.0714 -> 0.0740)
    a, b, c = -c0 / np.log2(np.e), -c1 / np.log2(np.e), -c2 / np.log2(np.e)
    assert abs(a - 1.595) < 2e-3 and abs(b - 0.074) < 2e-3 and -1e-3 < c < 0


def test_persistent_gemm_operand_bound_is_reported_by_the_supported_queries():
    """The persistent kernel reads A and W through 32-bit buffer descriptors reaching up to 255 rows past the last one: the `supported` queries the host
    asks before it plans a LayerNorm fold or a row-sum hand-over say no for operands that, padded to whole tiles, reach 4 GiB (pure host arithmetic).
    Pinned over _GEMM_QUERIES for wg_gemm_ln_supported, wg_gemm_row_partials_supported and wg_gemm_skinny_ln_supported."""
    assert _gemm_query_mismatches([5, 6, 7]) == []

_P = 1 << 20   # a 16-byte aligned address: every call below is refused before it could be used
_GEMM_ENTRY_ARGS = {   # parameter names (include/walkgpt_hip.h) and arguments every row below spoils in one place
    "wg_gemm_bias_act_bf16": ("A lda W ldw bias residual ldr res_row_mod C ldc M N K act out_f32 tile_hint stream",
                              (_P, 1024, _P, 1024, None, None, 0, 0, _P, 1024, 4096, 1024, 1024, 0, 0, 0, None)),
    "wg_gemm_skinny_ln_bias_act_bf16": ("A lda gamma beta eps W ldw w_tiled bias C ldc M N K act out_f32 stream",
                                        (_P, 256, None, None, 1e-5, _P, 256, 0, None, _P, 256, 8, 256, 256, 0, 0, None)),
    "wg_gemm_ln_bias_act_bf16": ("A lda Wg ldw bias_f32 colsum stats C ldc M N K act stream",
                                 (_P, 768, _P, 768, _P, _P, _P, _P, 2304, 32768, 2304, 768, 0, None)),
    "wg_gemm_lnp_bias_act_bf16": ("A lda Wg ldw bias_f32 colsum row_partials n_partials mpad eps C ldc M N K act stream",
                                  (_P, 768, _P, 768, _P, _P, _P, 3, 32768, 1e-5, _P, 2304, 32768, 2304, 768, 0, None)),
    "wg_gemm_bias_act_stats_bf16": ("A lda W ldw bias residual ldr res_row_mod C ldc M N K act row_partials mpad stream",
                                    (_P, 768, _P, 768, None, None, 0, 0, _P, 768, 32768, 768, 768, 0, _P, 32768, None)),
    "wg_gemm_mxfp8": ("Aq lda a_mx a_pitch Wq ldw w_mx w_pitch bias ln_colsum ln_bias ln_part ln_np ln_mpad ln_eps residual ldr res_row_mod "
                      "C ldc Cq ldcq c_mx c_pitch stats_part stats_mpad M N K act stream",
                      (_P, 1024, _P, 4096, _P, 1024, _P, 1024, None, None, None, None, 0, 0, 0.0, None, 0, 0,
                       _P, 1024, None, 0, None, 0, None, 0, 4096, 1024, 1024, 0, None)),
    "wg_gemm_fp8_bias_act": ("Aq lda scale_a Wq ldw scale_w bias residual ldr res_row_mod C ldc M N K act stream",
                             (_P, 1024, _P, _P, 1024, _P, None, None, 0, 0, _P, 1024, 4096, 1024, 1024, 0, None)),
}
_GEMM_REJECTS = [   # (entry point, spoiled arguments, prefix of wg_last_error())
    ("wg_gemm_bias_act_bf16", dict(W=None), "gemm: "),
    ("wg_gemm_bias_act_bf16", dict(M=0), "gemm: "),
    ("wg_gemm_bias_act_bf16", dict(ldc=1000), "gemm: "),
    ("wg_gemm_bias_act_bf16", dict(act=4), "gemm: "),
    ("wg_gemm_bias_act_bf16", dict(residual=_P, ldr=512), "gemm: "),   # (misaligned operands are not refused: they take the row-wave kernel)
    ("wg_gemm_skinny_ln_bias_act_bf16", dict(gamma=_P), "gemm_skinny: "),
    ("wg_gemm_skinny_ln_bias_act_bf16", dict(gamma=_P + 8, beta=_P), "gemm_skinny: "),
    ("wg_gemm_skinny_ln_bias_act_bf16", dict(W=_P + 8), "gemm_skinny: "),
    ("wg_gemm_skinny_ln_bias_act_bf16", dict(M=129), "gemm_skinny: "),
    ("wg_gemm_skinny_ln_bias_act_bf16", dict(K=192, lda=192, ldw=192), "gemm_skinny: "),
    ("wg_gemm_skinny_ln_bias_act_bf16", dict(A=None), "gemm: "),
    ("wg_gemm_ln_bias_act_bf16", dict(colsum=None), "gemm_ln: "),
    ("wg_gemm_ln_bias_act_bf16", dict(stats=_P + 8), "gemm_ln: "),
    ("wg_gemm_ln_bias_act_bf16", dict(C=_P + 8), "gemm_ln: "),
    ("wg_gemm_ln_bias_act_bf16", dict(M=100), "gemm_ln: "),
    ("wg_gemm_ln_bias_act_bf16", dict(ldc=2300), "gemm_ln: "),
    ("wg_gemm_lnp_bias_act_bf16", dict(row_partials=None), "gemm_lnp: "),
    ("wg_gemm_lnp_bias_act_bf16", dict(bias_f32=_P + 4), "gemm_lnp: "),
    ("wg_gemm_lnp_bias_act_bf16", dict(n_partials=2), "gemm_lnp: "),
    ("wg_gemm_lnp_bias_act_bf16", dict(mpad=32000), "gemm_lnp: "),
    ("wg_gemm_lnp_bias_act_bf16", dict(M=100, mpad=256), "gemm_lnp: "),
    ("wg_gemm_bias_act_stats_bf16", dict(row_partials=None), "gemm_stats: "),
    ("wg_gemm_bias_act_stats_bf16", dict(bias=_P + 8), "gemm_stats: "),
    ("wg_gemm_bias_act_stats_bf16", dict(N=1536, ldc=1536), "gemm_stats: "),
    ("wg_gemm_bias_act_stats_bf16", dict(mpad=32000), "gemm_stats: "),
    # a residual spanning 2 GiB or more cannot take the staged epilogue the row partials need
    ("wg_gemm_bias_act_stats_bf16", dict(residual=_P, ldr=1 << 20), "gemm: "),
    ("wg_gemm_mxfp8", dict(w_mx=None), "gemm_mxfp8: "),
    ("wg_gemm_mxfp8", dict(Aq=_P + 8), "gemm_mxfp8: "),
    ("wg_gemm_mxfp8", dict(K=192, lda=192, ldw=192), "gemm_mxfp8: "),
    ("wg_gemm_mxfp8", dict(ldc=1 << 20), "gemm_mxfp8: "),
    ("wg_gemm_mxfp8", dict(residual=_P, ldr=1 << 20), "gemm_mxfp8: "),
    ("wg_gemm_mxfp8", dict(Cq=_P, ldcq=1 << 20, c_mx=_P, c_pitch=4096), "gemm_mxfp8: "),
    ("wg_gemm_fp8_bias_act", dict(scale_w=None), "gemm_fp8: "),
    ("wg_gemm_fp8_bias_act", dict(bias=_P + 4), "gemm_fp8: "),
    ("wg_gemm_fp8_bias_act", dict(N=1004), "gemm_fp8: "),
    ("wg_gemm_fp8_bias_act", dict(ldc=1 << 20), "gemm_fp8: "),
]


def test_gemm_entry_points_refuse_bad_arguments_before_any_hip_call():
    """Every GEMM entry point refuses a null operand, a misaligned pointer and a shape it does not take with WG_ERR_BAD_ARG, before it
    touches the device, and names itself in wg_last_error()."""
    from walkgpt_amd import _lib
    L = _lib.lib()
    bad = []
    for entry, spoil, prefix in _GEMM_REJECTS:
        names, base = _GEMM_ENTRY_ARGS[entry]
        names = names.split()
        assert set(spoil) <= set(names) and len(names) == len(base)
        rc = getattr(L, entry)(*[spoil.get(n, v) for n, v in zip(names, base)])
        msg = L.wg_last_error().decode()
        if rc != -1 or not msg.startswith(prefix):
            bad.append((entry, spoil, rc, msg))
    assert bad == []


def test_rows_hand_out_by_products_only_while_x_is_unedited():
    """ops.Rows, the value that carries a GEMM's by-products to the next one: a fresh one hands them out, one whose x was edited in place
    through torch hands out none, and nothing is ever stored on the tensor object itself."""
    from walkgpt_amd import ops
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    part, pair = torch.zeros(1, 256, 2), (torch.zeros(4, 256, dtype=torch.uint8), torch.zeros(8, 256, dtype=torch.uint8))
    r = ops.Rows(x, part, pair)
    assert r.x is x and r.fresh() == (part, pair) and r.fresh()[0] is part and r.fresh()[1] is pair
    assert ops.Rows(x).fresh() == (None, None)
    assert not hasattr(r, "__dict__") and x.__dict__ == {}
    r.x.add_(1)
    assert r.fresh() == (None, None)
    assert ops.Rows(x, part, pair).fresh() == (part, pair)          # made after the edit: describes the tensor as it is now
    only_mx = ops.Rows(mx=pair)
    assert only_mx.x is None and only_mx.partials is None and only_mx.fresh() == (None, pair)
    assert x.__dict__ == {}
