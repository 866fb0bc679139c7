"""A straightforward composition of SamAutomaticMaskGenerator from SamPredictor.predict_torch(return_logits=True), torch thresholds and boxes, a
torch greedy NMS and the numpy RLE of amg.py's formula: what the reference's generator does (automatic_mask_generator.py:189-321), with every
full-resolution tensor it builds.  tests/test_gpu_amg.py holds SamAutomaticMaskGenerator.generate to it record by record, and tools/bench_amg.py
times it beside the fused path.  It sees the same logits as the generator, so nothing may differ.

Shared with the code under test, hence not checked by this comparison: generate_crop_boxes and is_box_near_crop_edge (imported from utils/amg.py;
both are held to the reference's outputs on CPU by tests/test_amg_host.py) and the fl32(p + 0.5) - 0.5 preparation of the points (repeated here
so that both paths decode the same prompts; the reference's fixture run pins it end to end)."""
import numpy as np
import torch

from walkgpt_amd.segment_anything.utils.amg import generate_crop_boxes, is_box_near_crop_edge


def mask_to_box(masks):
    """batched_mask_to_box (amg.py:303-346) for bool [N, H, W]: XYXY in inclusive pixel indices, zeros for an empty mask."""
    n, h, w = masks.shape
    rows, cols = masks.any(-1), masks.any(-2)
    ys, xs = torch.arange(h, device=masks.device)[None], torch.arange(w, device=masks.device)[None]
    bottom, top = (rows * ys).max(-1)[0], (rows * ys + h * (~rows)).min(-1)[0]
    right, left = (cols * xs).max(-1)[0], (cols * xs + w * (~cols)).min(-1)[0]
    empty = (right < left) | (bottom < top)
    return torch.stack([left, top, right, bottom], -1) * (~empty)[:, None]


def greedy_nms(boxes, scores, thr):
    """torchvision's CPU rule in plain torch: stable descending sort, suppress at iou > thr, area (x2 - x1)(y2 - y1)."""
    if boxes.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64)
    boxes, scores = boxes.float().cpu(), scores.float().cpu()
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
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
        removed[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > thr
    return torch.tensor(keep, dtype=torch.int64)


def rle_numpy(mask):
    """mask_to_rle_pytorch (amg.py:107-135) of one bool [H, W] array."""
    h, w = mask.shape
    flat = mask.transpose().reshape(-1)
    idx = np.concatenate([[0], np.flatnonzero(flat[1:] ^ flat[:-1]) + 1, [h * w]])
    counts = [] if not flat[0] else [0]
    counts.extend(np.diff(idx).tolist())
    return {"size": [h, w], "counts": counts}


@torch.no_grad()
def post_decoder(masks, iou_preds, points, thr, offset, pred_iou_thresh, stability_score_thresh, crop_box, orig_size):
    """automatic_mask_generator.py:283-321 on full-resolution logits [N, h, w]: (rles, iou, points, stability, boxes) of the survivors."""
    orig_h, orig_w = orig_size
    keep = torch.ones_like(iou_preds, dtype=torch.bool)
    if pred_iou_thresh > 0.0:
        keep &= iou_preds > pred_iou_thresh
    inter = (masks > (thr + offset)).sum((-1, -2), dtype=torch.int32)
    union = (masks > (thr - offset)).sum((-1, -2), dtype=torch.int32)
    stability = inter / union
    if stability_score_thresh > 0.0:
        keep &= stability >= stability_score_thresh
    binary = masks > thr
    boxes = mask_to_box(binary)
    keep &= ~is_box_near_crop_edge(boxes, crop_box, [0, 0, orig_w, orig_h])
    idx = torch.nonzero(keep).reshape(-1)
    x0, y0, x1, y1 = crop_box
    padded = torch.nn.functional.pad(binary[idx], (x0, orig_w - x1, y0, orig_h - y1), value=0)
    rles = [rle_numpy(m) for m in padded.cpu().numpy()]
    return rles, iou_preds[idx], points[idx.cpu()], stability[idx], boxes[idx]


@torch.no_grad()
def generate(predictor, image, point_grids, points_per_batch, pred_iou_thresh, stability_score_thresh, stability_score_offset, box_nms_thresh,
             crop_n_layers, crop_nms_thresh, crop_overlap_ratio, timer=None):
    """The records of SamAutomaticMaskGenerator.generate(image) in output_mode "uncompressed_rle"."""
    orig_size = image.shape[:2]
    dev = predictor.device
    thr = predictor.model.mask_threshold
    crop_boxes, layers = generate_crop_boxes(orig_size, crop_n_layers, crop_overlap_ratio)
    parts = []
    for crop_box, layer in zip(crop_boxes, layers):
        x0, y0, x1, y1 = crop_box
        crop = image[y0:y1, x0:x1, :]
        size = crop.shape[:2]
        predictor.set_image(crop)
        grid = point_grids[layer] * np.array(size)[None, ::-1]
        rles, ious, pts, stabs, boxes = [], [], [], [], []
        for b in range(0, len(grid), points_per_batch):
            points = grid[b:b + points_per_batch]
            shifted = torch.as_tensor(predictor.transform.apply_coords(points, size), dtype=torch.float64) + 0.5    # the prompt encoder's double add
            in_points = (shifted.to(torch.float32) - 0.5).to(dev)
            labels = torch.ones(len(points), dtype=torch.int, device=dev)
            masks, iou, _ = predictor.predict_torch(in_points[:, None, :], labels[:, None], multimask_output=True, return_logits=True)
            if timer is not None:
                timer("decoded")
            r = post_decoder(masks.flatten(0, 1), iou.flatten(0, 1), torch.as_tensor(points.repeat(masks.shape[1], axis=0)), thr, stability_score_offset,
                             pred_iou_thresh, stability_score_thresh, crop_box, orig_size)
            if timer is not None:
                timer("post")
            for acc, v in zip((rles, ious, pts, stabs, boxes), r):
                acc.append(v)
        predictor.reset_image()
        rles = [r for part in rles for r in part]
        ious, pts, stabs, boxes = torch.cat(ious), torch.cat(pts), torch.cat(stabs), torch.cat(boxes)
        keep = greedy_nms(boxes, ious, box_nms_thresh)
        kd = keep.to(dev)
        parts.append(dict(rles=[rles[i] for i in keep.tolist()], iou=ious[kd], points=pts[keep] + torch.tensor([[x0, y0]]), stability=stabs[kd],
                          boxes=boxes[kd] + torch.tensor([[x0, y0, x0, y0]], device=dev),
                          crop_boxes=torch.tensor([crop_box] * len(keep), dtype=torch.int64).reshape(-1, 4)))
    rles = [r for p in parts for r in p["rles"]]
    cat = {k: torch.cat([p[k] for p in parts]) for k in ("iou", "points", "stability", "boxes", "crop_boxes")}
    order = torch.arange(len(rles))
    if len(crop_boxes) > 1 and len(rles) > 0:
        cb = cat["crop_boxes"]
        order = greedy_nms(cat["boxes"], 1 / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])), crop_nms_thresh)
    out = []
    for i in order.tolist():
        box, cb = cat["boxes"][i].cpu().numpy(), cat["crop_boxes"][i].numpy()
        out.append({"segmentation": rles[i], "area": int(sum(rles[i]["counts"][1::2])),
                    "bbox": [box[0], box[1], box[2] - box[0], box[3] - box[1]],
                    "predicted_iou": cat["iou"][i].item(), "point_coords": [cat["points"][i].tolist()], "stability_score": cat["stability"][i].item(),
                    "crop_box": [cb[0], cb[1], cb[2] - cb[0], cb[3] - cb[1]]})
    return out
