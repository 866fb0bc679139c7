"""Host-side checks of SamAutomaticMaskGenerator: the public names, the C-ABI declarations, the helpers of utils/amg.py against the reference's
own outputs (tests/golden/amg_host_h1.npz), the counts-from-positions step, and the errors raised before any kernel runs."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.golden import cases, cases_amg as ca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wg_amg_mask_stats_f32", "wg_amg_rle_count_i32", "wg_amg_rle_write_i32", "wg_nms_f32")
NEW_QUERIES = ("wg_amg_mask_stats_workspace_ints", "wg_nms_workspace_words")


@pytest.fixture(scope="module")
def gold():
    return cases.load("amg_host_h1")


def test_generator_is_exported_under_all_three_names():
    from model.segment_anything import SamAutomaticMaskGenerator as A
    from walkgpt_amd.segment_anything import SamAutomaticMaskGenerator as B
    from walkgpt_amd.segment_anything.automatic_mask_generator import SamAutomaticMaskGenerator as C
    assert A is B is C
    assert callable(A.generate) and callable(A.postprocess_small_regions)
    p = inspect.signature(A.__init__).parameters
    want = dict(points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0,
                box_nms_thresh=0.7, crop_n_layers=0, crop_nms_thresh=0.7, crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=1,
                point_grids=None, min_mask_region_area=0, output_mode="binary_mask")
    assert list(p)[:2] == ["self", "model"] and list(p)[2:] == list(want)
    for k, v in want.items():
        assert p[k].default == v, k


def test_header_and_ctypes_table_declare_the_new_entry_points():
    txt = open(os.path.join(ROOT, "include", "walkgpt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from walkgpt_amd import _lib
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    for name in NEW_QUERIES:
        assert re.search(r"\blong\s+%s\s*\(" % name, code), name
        assert name in _lib.exported_symbols()
    # symbols were added, no argument list changed: the version stays
    api = open(os.path.join(ROOT, "walkgpt_amd", "csrc", "wg_api.hip")).read()
    assert re.search(r"wg_version\(void\)\s*\{\s*return 300;", api)
    # one copy of the postprocess arithmetic, included by both kernels' files
    csrc = os.path.join(ROOT, "walkgpt_amd", "csrc")
    for f in ("misc.hip", "amg.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "post_common.h"' in src and "v_mul_f32" not in src, f


def test_point_grids_crop_boxes_and_edge_filter_equal_the_reference(gold):
    from walkgpt_amd.segment_anything.utils import amg
    c = ca.HOST
    grids = amg.build_all_layer_point_grids(*c["grid"])
    assert len(grids) == c["grid"][1] + 1
    for i, g in enumerate(grids):
        assert g.dtype == np.float64 and np.array_equal(g, gold["grid%d" % i])
    boxes, layers = amg.generate_crop_boxes(c["frame"], c["crop_layers"], c["overlap"])
    assert np.array_equal(np.array(boxes), gold["crop_boxes"]) and np.array_equal(np.array(layers), gold["crop_layers"])
    assert len(boxes) == 1 + 4 + 16
    edge = amg.is_box_near_crop_edge(torch.tensor(ca.EDGE_BOXES), ca.EDGE_CROP, ca.EDGE_ORIG)
    assert np.array_equal(edge.numpy(), gold["edge"])
    assert 0 < int(gold["edge"].sum()) < len(ca.EDGE_BOXES)


def _placements():
    c = ca.HOST
    H, W = c["rle_frame"]
    h, w = c["rle_crop"]
    out = [("rle_crop_%d_%d" % (x0, y0), ca.rle_patterns(h, w), x0, y0) for x0, y0 in c["rle_offsets"]]
    return out + [("rle_full", ca.rle_patterns(H, W), 0, 0)], (H, W)


def test_counts_from_positions_reproduce_the_reference_rles(gold):
    """ops.rle_from_positions (the host half of ops.amg_rle) fed with change positions computed in numpy from the stored masks."""
    from walkgpt_amd import ops
    from walkgpt_amd.segment_anything.utils import amg
    placements, (H, W) = _placements()
    for key, masks, x0, y0 in placements:
        frames = [ca.place(m, x0, y0, H, W) for m in masks]
        pos = [ca.positions_numpy(f) for f in frames]
        rles = ops.rle_from_positions(np.concatenate(pos).astype(np.int32), np.cumsum([len(p) for p in pos]), [int(f[0, 0]) for f in frames], (H, W))
        want = ca.unpad_lists(gold[key], gold[key + "_len"])
        assert [r["counts"] for r in rles] == want, key
        for r, f in zip(rles, frames):
            assert r["size"] == [H, W] and sum(r["counts"]) == H * W
            assert np.array_equal(amg.rle_to_mask(r), f)
            assert amg.mask_to_rle_numpy(f) == r
            assert amg.area_from_rle(r) == int(f.sum())


def test_pack_bits_round_trip():
    m = ca.rle_patterns(70, 45)
    bits = ca.pack_bits(m)
    assert bits.shape == (6, 3, 45) and bits.dtype == np.int32
    assert np.array_equal(ca.unpack_bits(bits, 70), m)
    assert bits[2, 0, 0] == 1 and bits[3, 2, 44] == 1 << 5          # row 69 = word 2, bit 5


def test_remove_small_regions_on_hand_made_masks():
    from walkgpt_amd.segment_anything.utils.amg import remove_small_regions
    m = np.zeros((12, 12), dtype=bool)
    m[2:9, 2:9] = True
    holed = m.copy()
    holed[4:6, 4:6] = False                                   # a 4-pixel hole
    out, changed = remove_small_regions(holed, 5, "holes")
    assert changed and np.array_equal(out, m)
    out, changed = remove_small_regions(holed, 4, "holes")    # `<`, not `<=`
    assert not changed and out is holed
    island = m.copy()
    island[10, 10] = True
    island[11, 11] = True                                     # diagonal neighbours: ONE island of two under 8-connectivity
    out, changed = remove_small_regions(island, 3, "islands")
    assert changed and np.array_equal(out, m)
    out, changed = remove_small_regions(island, 2, "islands")
    assert not changed
    out, changed = remove_small_regions(m, 10, "islands")     # nothing to change
    assert not changed and out is m
    out, changed = remove_small_regions(m, 10, "holes")
    assert not changed
    small = np.zeros((12, 12), dtype=bool)
    small[1, 1:4] = True
    small[8, 2:4] = True
    out, changed = remove_small_regions(small, 100, "islands")      # every region is small: the largest stays
    want = np.zeros((12, 12), dtype=bool)
    want[1, 1:4] = True
    assert changed and np.array_equal(out, want)


def test_constructor_assertions_match_the_reference():
    from walkgpt_amd.segment_anything import SamAutomaticMaskGenerator
    with pytest.raises(AssertionError, match="Exactly one of points_per_side or point_grid must be provided."):
        SamAutomaticMaskGenerator(None, points_per_side=8, point_grids=[np.zeros((1, 2))])
    with pytest.raises(AssertionError, match="Exactly one of points_per_side or point_grid must be provided."):
        SamAutomaticMaskGenerator(None, points_per_side=None, point_grids=None)
    with pytest.raises(AssertionError, match="Unknown output_mode polygons."):
        SamAutomaticMaskGenerator(None, output_mode="polygons")


def _tiny_sam():
    from walkgpt_amd.segment_anything.modeling import ImageEncoderViT, MaskDecoder, PromptEncoder, Sam, TwoWayTransformer
    return Sam(image_encoder=ImageEncoderViT(img_size=64, embed_dim=64, depth=1, num_heads=1, use_rel_pos=True, window_size=0),
               prompt_encoder=PromptEncoder(embed_dim=256, image_embedding_size=(4, 4), input_image_size=(64, 64), mask_in_chans=16),
               mask_decoder=MaskDecoder(num_multimask_outputs=3, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                                        transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256))


def test_generate_has_no_cpu_fallback():
    from walkgpt_amd import _lib, ops
    from walkgpt_amd.segment_anything import SamAutomaticMaskGenerator
    gen = SamAutomaticMaskGenerator(_tiny_sam(), points_per_side=2)
    assert len(gen.point_grids) == 1 and gen.point_grids[0].shape == (4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gen.generate(np.zeros((40, 50, 3), dtype=np.uint8))
    with pytest.raises(_lib.WalkgptHipError):
        ops.amg_mask_stats(torch.zeros(1, 8, 8), 32, (32, 32), (40, 40), 0.0, 1.0)
    with pytest.raises(_lib.WalkgptHipError):
        ops.nms(torch.zeros(2, 4), torch.zeros(2), 0.5)
    with pytest.raises(_lib.WalkgptHipError):
        ops.amg_rle(torch.zeros(1, 1, 8, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), [0, 0, 8, 8], (8, 8))


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    import __graft_entry__ as ge
    ge.build()
    from walkgpt_amd import _lib
    h = _lib.lib()
    assert h.wg_amg_mask_stats_workspace_ints(70, 33, 257) == 70 * 2 * 2 * 8
    assert h.wg_nms_workspace_words(65) == 65 * 2
    assert h.wg_amg_mask_stats_f32(None, None, None, None, 0, 1, 8, 8, 32, 32, 32, 8, 8, 0.0, 1.0, None) < 0 and b"amg_mask_stats" in h.wg_last_error()
    assert h.wg_nms_f32(1, 1, 0.5, 1, 1, 1, 1 << 30, 8193, None) < 0 and b"8192" in h.wg_last_error()
    assert h.wg_amg_rle_count_i32(1, 1, 1, 1, 1, 70, 45, 40, 13, 97, 76, None) < 0 and b"inside" in h.wg_last_error()
    assert h.wg_amg_rle_count_i32(1, 1, 1, 1, 1, 46341, 46341, 0, 0, 46341, 46341, None) < 0 and b"2^31" in h.wg_last_error()
    assert h.wg_amg_rle_write_i32(1, 1, None, 1, 0, 1, 1, 1, 8, 8, 0, 0, 8, 8, None) < 0


def test_amg_fixtures_are_small_and_complete():
    for name in ["amg_stats_%s" % k for k in ca.STATS] + ["amg_host_h1", "amg_e2e_b128"]:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < (1 << 20), name
    e = cases.load("amg_e2e_b128")
    assert 8 <= len(e["area"]) <= 64 and len(e["area_bf16"]) > 0
    for k in ("counts", "counts_len", "bbox", "predicted_iou", "stability_score", "point_coords", "crop_box"):
        assert k in e and k + "_bf16" in e, k
    for name, c in ca.STATS.items():
        d = cases.load("amg_stats_" + name)
        band = (d["cnt_out"] - d["cnt_in"]).max() / float(c["output"][0] * c["output"][1])
        assert band <= ca.BAND_MAX and d["exact"].shape == (c["n"], 7)
        assert (d["cnt_in"] <= d["exact"][:, :3]).all() and (d["exact"][:, :3] <= d["cnt_out"]).all()


def test_more_boxes_than_the_device_nms_takes_is_a_clear_error():
    from walkgpt_amd.segment_anything import automatic_mask_generator as G
    n = G.NMS_MAX_BOXES + 1
    with pytest.raises(RuntimeError, match="at most 8192"):
        G._nms(torch.zeros(n, 4), torch.zeros(n), 0.7, "across crops")
    sig = inspect.signature(G.SamAutomaticMaskGenerator.postprocess_small_regions)
    assert list(sig.parameters) == ["mask_data", "min_area", "nms_thresh", "device"] and sig.parameters["device"].default is None
