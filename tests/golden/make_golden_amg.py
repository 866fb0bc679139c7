"""Generate tests/golden/amg_stats_<case>.npz, amg_host_h1.npz and amg_e2e_b128.npz from the REFERENCE's own Sam.postprocess_masks, utils/amg.py
functions and SamAutomaticMaskGenerator (imported from the reference checkout through make_golden._import_reference) on the cases of
cases_amg.py, on CPU in fp32.  Only outputs are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_amg.py [stats] [host] [e2e] [explore]

torchvision is not installed: batched_nms and box_area are stood in by the plain-torch functions below (stable descending sort, greedy
suppression at iou > thr, area without +1 -- torchvision's CPU rule and arithmetic), assigned on the reference's modules the way
make_golden_prompts.py stands in `resize`.  `explore` prints the score distributions the thresholds of cases_amg.E2E were chosen from.
"""
import importlib
import os
import sys
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import cases_amg as ca, cases_prompts as cp  # noqa: E402
from tests.golden.make_golden import _import_reference  # noqa: E402


# ---- stand-ins for torchvision.ops.boxes -----------------------------------------------------------------------------------------------------
def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def nms(boxes, scores, iou_threshold):
    if boxes.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order]
    area = box_area(b)
    removed = torch.zeros(b.shape[0], dtype=torch.bool)
    keep = []
    for i in range(b.shape[0]):
        if removed[i]:
            continue
        keep.append(int(order[i]))
        r = b[i + 1:]
        w = (torch.minimum(b[i, 2], r[:, 2]) - torch.maximum(b[i, 0], r[:, 0])).clamp(min=0)
        h = (torch.minimum(b[i, 3], r[:, 3]) - torch.maximum(b[i, 1], r[:, 1])).clamp(min=0)
        inter = w * h
        removed[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > iou_threshold
    return torch.tensor(keep, dtype=torch.int64)


def batched_nms(boxes, scores, idxs, iou_threshold):
    assert bool((idxs == 0).all()), "the generator passes one category"
    return nms(boxes.float(), scores.float(), iou_threshold)


def _reference_amg():
    sam_modeling, _ = _import_reference()
    tvb = sys.modules["torchvision.ops.boxes"]
    tvb.batched_nms, tvb.box_area = batched_nms, box_area
    amg = importlib.import_module("model.segment_anything.utils.amg")
    assert amg.__file__.startswith("/root/reference")
    return sam_modeling, amg


def _box(mask):
    ys, xs = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
    return [0, 0, 0, 0] if ys.size == 0 else [xs[0], ys[0], xs[-1], ys[-1]]


# ---- amg_stats_<case>.npz -------------------------------------------------------------------------------------------------------------------
def make_stats(name):
    sam_modeling, amg = _reference_amg()
    c = ca.STATS[name]
    fake_sam = SimpleNamespace(image_encoder=SimpleNamespace(img_size=c["img"]))
    for attempt in range(8):
        low = torch.from_numpy(ca.stats_logits(c, attempt))
        with torch.no_grad():
            ref = sam_modeling.Sam.postprocess_masks(fake_sam, low[:, None], c["input"], c["output"])[:, 0]
        delta = ca.stats_delta(float(ref.abs().max()))
        ts = (ca.THR + ca.OFF, ca.THR - ca.OFF, ca.THR)
        r = ref.numpy()
        cnt_in = np.stack([(r > t + delta).sum((1, 2)) for t in ts], 1)        # the fewest pixels a count may have
        cnt_out = np.stack([(r > t - delta).sum((1, 2)) for t in ts], 1)       # the most
        band = (cnt_out - cnt_in).max() / float(r.shape[1] * r.shape[2])
        print("  stats %s attempt %d: delta %.3g, widest band %.4f %% of the frame, bands of zero: %d of %d masks" % (
            name, attempt, delta, 100 * band, int(((cnt_out - cnt_in).sum(1) == 0).sum()), r.shape[0]))
        if band <= ca.BAND_MAX:
            break
    else:
        raise AssertionError("no seed keeps the band below %.2f %%" % (100 * ca.BAND_MAX))
    exact = np.concatenate([np.stack([(r > t).sum((1, 2)) for t in ts], 1), amg.batched_mask_to_box(ref > ca.THR).numpy()], 1)
    stab = amg.calculate_stability_score(ref, ca.THR, ca.OFF).numpy()
    np.savez_compressed(os.path.join(HERE, "amg_stats_%s.npz" % name), attempt=np.int64(attempt), delta=np.float64(delta), cnt_in=cnt_in,
                        cnt_out=cnt_out, box_in=np.array([_box(m > ca.THR + delta) for m in r]), box_out=np.array([_box(m > ca.THR - delta) for m in r]),
                        exact=exact.astype(np.int64), stability=stab)


# ---- amg_host_h1.npz ------------------------------------------------------------------------------------------------------------------------
def make_host():
    _, amg = _reference_amg()
    c = ca.HOST
    out = {}
    for i, g in enumerate(amg.build_all_layer_point_grids(*c["grid"])):
        out["grid%d" % i] = g
    boxes, layers = amg.generate_crop_boxes(c["frame"], c["crop_layers"], c["overlap"])
    out["crop_boxes"], out["crop_layers"] = np.array(boxes), np.array(layers)
    out["edge"] = amg.is_box_near_crop_edge(torch.tensor(ca.EDGE_BOXES), ca.EDGE_CROP, ca.EDGE_ORIG).numpy()
    H, W = c["rle_frame"]
    h, w = c["rle_crop"]
    crop = torch.from_numpy(ca.rle_patterns(h, w))
    for x0, y0 in c["rle_offsets"]:
        rles = amg.mask_to_rle_pytorch(amg.uncrop_masks(crop, [x0, y0, x0 + w, y0 + h], H, W))
        assert all(r["size"] == [H, W] for r in rles)
        out["rle_crop_%d_%d" % (x0, y0)], out["rle_crop_%d_%d_len" % (x0, y0)] = ca.pad_lists([r["counts"] for r in rles])
    full = torch.from_numpy(ca.rle_patterns(H, W))
    rles = amg.mask_to_rle_pytorch(amg.uncrop_masks(full, [0, 0, W, H], H, W))
    out["rle_full"], out["rle_full_len"] = ca.pad_lists([r["counts"] for r in rles])
    b, s, tied = (torch.from_numpy(v) for v in ca.nms_boxes(c))
    for thr in c["nms_thresholds"]:
        out["nms_%g" % thr] = batched_nms(b, s, torch.zeros(len(b)), thr).numpy()
        out["nms_tied_%g" % thr] = batched_nms(b, tied, torch.zeros(len(b)), thr).numpy()
        for n in (1, 64, 65):
            out["nms_n%d_%g" % (n, thr)] = batched_nms(b[:n], s[:n], torch.zeros(n), thr).numpy()
        print("  host nms at %g: %d of %d kept, %d with tied scores" % (thr, len(out["nms_%g" % thr]), len(b), len(out["nms_tied_%g" % thr])))
    np.savez_compressed(os.path.join(HERE, "amg_host_h1.npz"), **out)


# ---- amg_e2e_b128.npz -----------------------------------------------------------------------------------------------------------------------
def _build_generator(bf16, **kw):
    from PIL import Image
    sam_modeling, amg = _reference_amg()
    tvf = sys.modules["torchvision.transforms.functional"]
    tvf.to_pil_image = lambda a: Image.fromarray(a)
    tvf.resize = lambda im, size: im.resize((size[1], size[0]), Image.BILINEAR)
    tr = importlib.import_module("model.segment_anything.utils.transforms")
    tr.to_pil_image, tr.resize = tvf.to_pil_image, tvf.resize
    gen_mod = importlib.import_module("model.segment_anything.automatic_mask_generator")
    gen_mod.batched_nms, gen_mod.box_area = batched_nms, box_area
    c = cp.PREDICTORS[ca.E2E["predictor"]]
    S = c["image_size"]
    g = S // 16
    sam = sam_modeling.Sam(
        image_encoder=sam_modeling.ImageEncoderViT(depth=c["depth"], embed_dim=c["embed_dim"], img_size=S, mlp_ratio=4,
                                                   norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_heads=c["heads"], patch_size=16, qkv_bias=True,
                                                   use_rel_pos=True, global_attn_indexes=c["global_idx"], window_size=14, out_chans=256),
        prompt_encoder=sam_modeling.PromptEncoder(embed_dim=256, image_embedding_size=(g, g), input_image_size=(S, S), mask_in_chans=16),
        mask_decoder=sam_modeling.MaskDecoder(num_multimask_outputs=3, transformer=sam_modeling.TwoWayTransformer(
            depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8), transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256))
    sam.load_state_dict(cp.predictor_state_dict(c, sam), strict=True)
    sam.eval()
    fwd = sam.prompt_encoder.forward
    sam.prompt_encoder.forward = lambda points, boxes, masks, text_embeds=None: fwd(points, boxes, masks, text_embeds)
    if bf16:
        # the modules in bf16 (the PE matrix and the pixel statistics stay fp32, as in the build); what enters the encoder and the decoder is cast
        # to bf16, what leaves the decoder back to fp32
        keep = {n: getattr(sam, n).data.clone() for n in ("pixel_mean", "pixel_std")}
        G = sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data.clone()
        sam.bfloat16()
        for n, v in keep.items():
            getattr(sam, n).data = v
        sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data = G

        def to16(_, args, kwargs):
            cast = lambda v: v.bfloat16() if torch.is_tensor(v) and v.is_floating_point() else v  # noqa: E731
            return tuple(cast(a) for a in args), {k: cast(v) for k, v in kwargs.items()}

        sam.image_encoder.register_forward_pre_hook(to16, with_kwargs=True)
        sam.mask_decoder.register_forward_pre_hook(to16, with_kwargs=True)
        sam.mask_decoder.register_forward_hook(lambda _m, _a, out: tuple(o.float() for o in out))
    return gen_mod.SamAutomaticMaskGenerator(sam, **kw), cp.predictor_frame(c)


def _records(anns):
    return [([int(v) for v in a["crop_box"]], ca.rle_mask(a["segmentation"]["size"], a["segmentation"]["counts"])) for a in anns]


def explore():
    kw = dict(ca.e2e_kwargs(), pred_iou_thresh=0.0, stability_score_thresh=0.0)
    gen, frame = _build_generator(False, **kw)
    anns = gen.generate(frame)
    iou = np.array([a["predicted_iou"] for a in anns])
    stab = np.array([a["stability_score"] for a in anns])
    q = [0, 10, 25, 50, 75, 90, 100]
    print("  with no score filter: %d records; predicted_iou percentiles %s: %s; stability %s" % (
        len(anns), q, np.round(np.percentile(iou, q), 4), np.round(np.percentile(stab[~np.isnan(stab)], q), 4)))
    for pi in np.percentile(iou, [25, 50, 75]):
        for st in (0.5, 0.7, 0.8, 0.9):
            g2, _ = _build_generator(False, **dict(kw, pred_iou_thresh=float(pi), stability_score_thresh=st))
            print("    pred_iou_thresh %.4f stability_score_thresh %.2f -> %d records" % (pi, st, len(g2.generate(frame))))


def make_e2e():
    kw = ca.e2e_kwargs()
    out = {}
    recs = {}
    for tag, bf16 in (("", False), ("_bf16", True)):
        gen, frame = _build_generator(bf16, **kw)
        with torch.no_grad():
            anns = gen.generate(frame)
        recs[tag] = _records(anns)
        out["counts" + tag], out["counts_len" + tag] = ca.pad_lists([a["segmentation"]["counts"] for a in anns])
        out["bbox" + tag] = np.array([a["bbox"] for a in anns], dtype=np.int64).reshape(-1, 4)
        out["area" + tag] = np.array([a["area"] for a in anns], dtype=np.int64)
        out["predicted_iou" + tag] = np.array([a["predicted_iou"] for a in anns], dtype=np.float32)
        out["stability_score" + tag] = np.array([a["stability_score"] for a in anns], dtype=np.float32)
        out["point_coords" + tag] = np.array([a["point_coords"][0] for a in anns], dtype=np.float64).reshape(-1, 2)
        out["crop_box" + tag] = np.array([a["crop_box"] for a in anns], dtype=np.int64).reshape(-1, 4)
        print("  e2e%s: %d records, areas %d .. %d" % (tag, len(anns), out["area" + tag].min(), out["area" + tag].max()))
    assert 8 <= len(recs[""]) <= 64, "the thresholds of cases_amg.E2E keep %d records, not 8 .. 64" % len(recs[""])
    out["size"] = np.array(frame.shape[:2])
    out["cal_unmatched_fp32"] = np.float64(ca.unmatched_share(recs[""], recs["_bf16"])[0])      # fp32 records the bf16 run does not have
    out["cal_unmatched_bf16"] = np.float64(ca.unmatched_share(recs["_bf16"], recs[""])[0])      # and the other way round
    print("  e2e calibration: unmatched share fp32 -> bf16 %.3f, bf16 -> fp32 %.3f" % (out["cal_unmatched_fp32"], out["cal_unmatched_bf16"]))
    np.savez_compressed(os.path.join(HERE, "amg_e2e_b128.npz"), **out)


if __name__ == "__main__":
    want = sys.argv[1:]
    torch.set_num_threads(8)
    if "explore" in want:
        explore()
    if not want or "stats" in want:
        for name in ca.STATS:
            print("generating stats:%s" % name, flush=True)
            make_stats(name)
    if not want or "host" in want:
        print("generating host", flush=True)
        make_host()
    if not want or "e2e" in want:
        print("generating e2e", flush=True)
        make_e2e()
