"""GPU checks of SamAutomaticMaskGenerator's kernels (wg_amg_mask_stats_f32, wg_amg_rle_*_i32, wg_nms_f32) and of generate() end to end."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import amg_reference as ar
from tests.golden import cases, cases_amg as ca, cases_prompts as cp
from walkgpt_amd import _lib, ops
from walkgpt_amd.segment_anything import SamAutomaticMaskGenerator, SamPredictor
from walkgpt_amd.segment_anything import modeling as M
from walkgpt_amd.segment_anything.utils import amg

pytestmark = pytest.mark.gpu
_cache = {}


def _stats_case(name, dev):
    """(case, fixture, low-res logits on the device, our own postprocess of them, ops.amg_mask_stats of them), computed once per geometry."""
    if name not in _cache:
        c, gold = ca.STATS[name], cases.load("amg_stats_" + name)
        low = torch.from_numpy(ca.stats_logits(c, int(gold["attempt"]))).to(dev)
        post = ops.postprocess_masks(low[:, None].contiguous(), c["img"], c["input"], c["output"])[:, 0]
        stats, bits = ops.amg_mask_stats(low, c["img"], c["input"], c["output"], ca.THR, ca.OFF)
        torch.cuda.synchronize()
        _cache[name] = (c, gold, low, post, stats, bits)
    return _cache[name]


def _want_from_postprocess(post):
    counts = torch.stack([(post > t).sum((-1, -2), dtype=torch.int32) for t in (ca.THR + ca.OFF, ca.THR - ca.OFF, ca.THR)], 1)
    return counts, ar.mask_to_box(post > ca.THR).to(torch.int32), (post > ca.THR).cpu().numpy()


@pytest.mark.parametrize("name", list(ca.STATS))
def test_mask_stats_equal_our_own_postprocess(dev, name):
    """Counts, box and bits are those of the floats wg_postprocess_masks_f32 writes, exactly; N = 70 and N = 1; three calls, the same bits."""
    c, _, low, post, stats, bits = _stats_case(name, dev)
    H, W = c["output"]
    counts, boxes, binary = _want_from_postprocess(post)
    assert stats.shape == (c["n"], 8) and stats.dtype == torch.int32 and bits.shape == (c["n"], (H + 31) // 32, W)
    assert torch.equal(stats[:, :3], counts)
    assert torch.equal(stats[:, 3:7], boxes)
    assert int(stats[:, 7].abs().max()) == 0
    assert np.array_equal(ca.unpack_bits(bits.cpu().numpy(), H), binary)
    assert np.array_equal(ca.pack_bits(binary), bits.cpu().numpy()), "rows past out_h must be 0"
    # the constructed masks: empty (box 0,0,0,0), full, one low-res peak
    n = c["n"]
    assert stats[n - 3].tolist() == [0] * 8
    assert stats[n - 2].tolist() == [H * W, H * W, H * W, 0, 0, W - 1, H - 1, 0]
    assert 0 < int(stats[n - 1, 0]) <= int(stats[n - 1, 2]) <= int(stats[n - 1, 1]) < H * W // 4
    for _ in range(2):
        s2, b2 = ops.amg_mask_stats(low, c["img"], c["input"], c["output"], ca.THR, ca.OFF)
        assert torch.equal(s2, stats) and torch.equal(b2, bits)
    for i in (0, n - 1):
        s1, b1 = ops.amg_mask_stats(low[i:i + 1].contiguous(), c["img"], c["input"], c["output"], ca.THR, ca.OFF)
        assert torch.equal(s1, stats[i:i + 1]) and torch.equal(b1, bits[i:i + 1])


@pytest.mark.parametrize("name", list(ca.STATS))
def test_mask_stats_against_the_reference(dev, name):
    """Each count lies between the reference's counts at t + delta and t - delta, the box between the two boxes; where the band is empty the
    reference's exact statistics are met."""
    c, gold, _, _, stats, _ = _stats_case(name, dev)
    s = stats.cpu().numpy().astype(np.int64)
    assert (gold["cnt_in"] <= s[:, :3]).all() and (s[:, :3] <= gold["cnt_out"]).all()
    inner, outer = gold["box_in"], gold["box_out"]
    has_in, has_out = (gold["cnt_in"][:, 2] > 0), (gold["cnt_out"][:, 2] > 0)
    box = s[:, 3:7]
    assert (box[~has_out] == 0).all()
    assert (box[has_in, :2] <= inner[has_in, :2]).all() and (box[has_in, 2:] >= inner[has_in, 2:]).all()
    nonempty = s[:, 2] > 0
    assert (box[nonempty, :2] >= outer[nonempty, :2]).all() and (box[nonempty, 2:] <= outer[nonempty, 2:]).all()
    sure = (gold["cnt_out"] - gold["cnt_in"]).sum(1) == 0
    assert sure.sum() >= 3
    assert np.array_equal(s[sure, :7], gold["exact"][sure])
    stab = (stats[:, 0] / stats[:, 1]).cpu().numpy()
    assert np.array_equal(np.isnan(stab), np.isnan(gold["stability"])) and np.array_equal(stab[sure], gold["stability"][sure], equal_nan=True)


def _rle_placements():
    c = ca.HOST
    H, W = c["rle_frame"]
    h, w = c["rle_crop"]
    out = [("rle_crop_%d_%d" % (x0, y0), ca.rle_patterns(h, w), [x0, y0, x0 + w, y0 + h]) for x0, y0 in c["rle_offsets"]]
    return out + [("rle_full", ca.rle_patterns(H, W), [0, 0, W, H])], (H, W)


def test_rle_equals_the_reference(dev):
    """The six masks of amg_host, bit-packed on the host into the kernel's layout, cropped (inside the frame, touching its far sides, at its
    first pixel) and uncropped; a keep list that selects and reorders."""
    gold = cases.load("amg_host_h1")
    placements, frame = _rle_placements()
    for key, masks, crop_box in placements:
        bits = torch.from_numpy(ca.pack_bits(masks)).to(dev)
        want = ca.unpad_lists(gold[key], gold[key + "_len"])
        got = ops.amg_rle(bits, torch.arange(6, device=dev), crop_box, frame)
        assert [r["counts"] for r in got] == want, key
        assert all(r["size"] == list(frame) for r in got)
        pick = [4, 0, 2]
        got = ops.amg_rle(bits, torch.tensor(pick, device=dev, dtype=torch.int32), crop_box, frame)
        assert [r["counts"] for r in got] == [want[i] for i in pick], key
    assert ops.amg_rle(bits, torch.empty(0, dtype=torch.int64, device=dev), crop_box, frame) == []
    for bad in ([0, 6], [-1, 2]):                      # outside the six planes: refused, not clamped in silence
        with pytest.raises(_lib.WalkgptHipError, match="outside"):
            ops.amg_rle(bits, torch.tensor(bad, device=dev), crop_box, frame)


@pytest.mark.parametrize("name", list(ca.STATS))
def test_rle_of_the_stats_masks(dev, name):
    """area == sum(counts[1::2]) == stats[:, 2], and the code decodes to the thresholded postprocess output: in place and inside a larger frame."""
    c, _, _, post, stats, bits = _stats_case(name, dev)
    H, W = c["output"]
    binary = (post > ca.THR).cpu().numpy()
    keep = torch.arange(c["n"], device=dev)
    for crop_box, frame in (([0, 0, W, H], (H, W)), ([5, 3, 5 + W, 3 + H], (H + 3, W + 9)), ([0, 2, W, 2 + H], (H + 2, W))):
        rles = ops.amg_rle(bits, keep, crop_box, frame)
        assert [amg.area_from_rle(r) for r in rles] == stats[:, 2].tolist()
        for i in (0, 7, c["n"] - 3, c["n"] - 2, c["n"] - 1):
            assert rles[i] == ar.rle_numpy(ca.place(binary[i], crop_box[0], crop_box[1], *frame)), (crop_box, i)


def test_nms_equals_the_reference_rule(dev):
    gold = cases.load("amg_host_h1")
    b, s, tied = (torch.from_numpy(v).to(dev) for v in ca.nms_boxes())
    for thr in ca.HOST["nms_thresholds"]:
        keep = ops.nms(b, s, thr)
        assert keep.dtype == torch.int64 and keep.device.type == "cuda"
        assert keep.tolist() == gold["nms_%g" % thr].tolist()
        assert ops.nms(b, tied, thr).tolist() == gold["nms_tied_%g" % thr].tolist()
        for n in (1, 64, 65):
            assert ops.nms(b[:n].contiguous(), s[:n].contiguous(), thr).tolist() == gold["nms_n%d_%g" % (n, thr)].tolist(), n
        assert b[keep].shape == (len(keep), 4)            # indexes like torchvision's
    assert ops.nms(b[:0], s[:0], 0.5).shape == (0,)
    same = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 5, device=dev)
    assert ops.nms(same, torch.ones(5, device=dev), 0.5).tolist() == [0]          # equal scores: the first in input order survives
    assert ops.nms(same, torch.ones(5, device=dev), 1.0).tolist() == [0, 1, 2, 3, 4]   # iou == thr does not suppress


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _sam(dev):
    c = cp.PREDICTORS[ca.E2E["predictor"]]
    sam = M._build_sam(c["embed_dim"], c["depth"], c["heads"], c["global_idx"], image_size=c["image_size"])
    sam.load_state_dict(cp.predictor_state_dict(c, sam), strict=True)
    G = sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data.clone()
    mean, std = sam.pixel_mean.data.clone(), sam.pixel_std.data.clone()
    sam.to(dev).bfloat16()
    sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data = G.to(dev)     # fp32 buffers, as the reference's fp32 run has them
    sam.pixel_mean.data, sam.pixel_std.data = mean.to(dev), std.to(dev)
    return sam, cp.predictor_frame(c)


def _e2e(dev):
    if "e2e" not in _cache:
        sam, frame = _sam(dev)
        gen = SamAutomaticMaskGenerator(sam, **ca.e2e_kwargs())
        _cache["e2e"] = (sam, frame, gen, gen.generate(frame))
    return _cache["e2e"]


def test_generate_equals_the_plain_composition(dev):
    """generate() against tests/amg_reference.py on the same device: both see the same logits, so counts, boxes, areas and order are equal and
    the two scores are the same bits."""
    sam, frame, gen, ours = _e2e(dev)
    kw = ca.e2e_kwargs()
    want = ar.generate(SamPredictor(sam), frame, gen.point_grids, kw["points_per_batch"], kw["pred_iou_thresh"], kw["stability_score_thresh"], 1.0,
                       kw["box_nms_thresh"], kw["crop_n_layers"], kw["crop_nms_thresh"], 512 / 1500)
    assert len(ours) == len(want) and len(ours) >= 4
    # each score filter is live in this case (a threshold that is not > 0 switches its filter off in both generators): without it more survive,
    # and what it drops is what lies at or below the threshold
    for key, field in (("pred_iou_thresh", "predicted_iou"), ("stability_score_thresh", "stability_score")):
        assert kw[key] > 0.0 and all(r[field] > kw[key] if key == "pred_iou_thresh" else r[field] >= kw[key] for r in ours)
        loose = SamAutomaticMaskGenerator(sam, **dict(kw, **{key: 0.0})).generate(frame)
        assert len(loose) > len(ours) and min(r[field] for r in loose) <= kw[key], key
    for a, b in zip(ours, want):
        assert sorted(a) == ["area", "bbox", "crop_box", "point_coords", "predicted_iou", "segmentation", "stability_score"]
        assert a["segmentation"] == b["segmentation"]
        assert a["area"] == b["area"] and isinstance(a["area"], int)
        assert a["bbox"] == [int(v) for v in b["bbox"]] and a["crop_box"] == [int(v) for v in b["crop_box"]]
        assert np.float32(a["predicted_iou"]).tobytes() == np.float32(b["predicted_iou"]).tobytes()
        assert np.float32(a["stability_score"]).tobytes() == np.float32(b["stability_score"]).tobytes()
        assert a["point_coords"] == b["point_coords"]


def _records(anns):
    return [([int(v) for v in a["crop_box"]], ca.rle_mask(a["segmentation"]["size"], a["segmentation"]["counts"])) for a in anns]


def test_generate_against_the_reference(dev):
    """Share of the reference's fp32 records that ours leave unmatched (same crop box, mask IoU >= 0.9) <= max(1.5 x the share the reference's own
    bf16 run leaves, 1 / number of records), and the other way round; matched pairs agree on point_coords and crop_box."""
    _, frame, _, ours = _e2e(dev)
    gold = cases.load("amg_e2e_b128")
    counts = ca.unpad_lists(gold["counts"], gold["counts_len"])
    size = [int(v) for v in gold["size"]]
    ref = [{"segmentation": {"size": size, "counts": counts[i]}, "crop_box": gold["crop_box"][i].tolist(),
            "point_coords": [gold["point_coords"][i].tolist()]} for i in range(len(counts))]
    assert size == list(frame.shape[:2])
    ro, rr = _records(ours), _records(ref)
    miss_ref, pairs = ca.unmatched_share(rr, ro)
    miss_ours, _ = ca.unmatched_share(ro, rr)
    print("unmatched: reference -> ours %.3f (calibration %.3f), ours -> reference %.3f (calibration %.3f); %d / %d records" % (
        miss_ref, float(gold["cal_unmatched_fp32"]), miss_ours, float(gold["cal_unmatched_bf16"]), len(ours), len(ref)))
    assert miss_ref <= max(1.5 * float(gold["cal_unmatched_fp32"]), 1.0 / len(rr))
    assert miss_ours <= max(1.5 * float(gold["cal_unmatched_bf16"]), 1.0 / max(len(ro), 1))
    for i, j in pairs:
        assert ref[i]["point_coords"] == ours[j]["point_coords"] and [int(v) for v in ref[i]["crop_box"]] == [int(v) for v in ours[j]["crop_box"]]


def test_binary_mask_mode_and_small_region_cleanup(dev):
    sam, frame, _, ours = _e2e(dev)
    gen = SamAutomaticMaskGenerator(sam, **dict(ca.e2e_kwargs(), output_mode="binary_mask"))
    masks = gen.generate(frame)
    assert len(masks) == len(ours)
    m = masks[0]["segmentation"]
    assert m.dtype == bool and m.shape == frame.shape[:2] and np.array_equal(m, amg.rle_to_mask(ours[0]["segmentation"]))
    assert int(m.sum()) == masks[0]["area"]
    # min_mask_region_area: every surviving mask is free of holes and islands below the area.  The one exception is the reference's own
    # (amg.py:287-289): where every island is below the area the largest stays, alone -- random weights give such speckled masks here
    area = 200
    cleaned = SamAutomaticMaskGenerator(sam, **dict(ca.e2e_kwargs(), output_mode="binary_mask", min_mask_region_area=area)).generate(frame)
    assert 0 < len(cleaned) <= len(ours)
    for r in cleaned:
        seg = r["segmentation"]
        assert not amg.remove_small_regions(seg, area, "holes")[1]
        again, changed = amg.remove_small_regions(seg, area, "islands")
        assert np.array_equal(again, seg)
        if changed:
            assert 0 < int(seg.sum()) < area and ndimage.label(seg, structure=np.ones((3, 3), dtype=bool))[1] == 1
        assert r["area"] == int(seg.sum())
        ys, xs = np.flatnonzero(seg.any(1)), np.flatnonzero(seg.any(0))
        assert r["bbox"] == [xs[0], ys[0], xs[-1] - xs[0], ys[-1] - ys[0]]
