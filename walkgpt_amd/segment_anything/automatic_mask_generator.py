"""SamAutomaticMaskGenerator of the reference (model/segment_anything/automatic_mask_generator.py) on the HIP path.

Same constructor arguments and defaults, same generate(image) records.  The reference materialises every mask of a batch at the frame's size
in fp32 and passes over it five times (stability score :296-300, threshold and boxes :306-307, RLE :317-318); here one kernel reads the
decoder's low-res logits and leaves the three counts, the box and the bit-packed mask (ops.amg_mask_stats), the filters run on that [N, 8]
tensor, the survivors' run-length codes come from the bits (ops.amg_rle), and NMS is ops.nms.  Inference-only; there is no CPU fallback.

Limit: the device NMS takes at most 8192 boxes per call (NMS_MAX_BOXES).  One crop with the default 32 x 32 points gives at most 3072, but the
NMS across crops (crop_n_layers >= 1) and the one of postprocess_small_regions see every crop's survivors together; generate raises a
RuntimeError that says so when they are more, instead of failing inside the library.
"""
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops
from .modeling import Sam
from .predictor import SamPredictor
from .utils.amg import (area_from_rle, batch_iterator, box_xyxy_to_xywh, build_all_layer_point_grids, coco_encode_rle, generate_crop_boxes,
                        is_box_near_crop_edge, mask_to_box_numpy, mask_to_rle_numpy, remove_small_regions, rle_to_mask, uncrop_boxes_xyxy,
                        uncrop_points)

_KEYS = ("iou_preds", "points", "stability_score", "boxes", "crop_boxes")
NMS_MAX_BOXES = 8192         # wg_nms_f32's limit per call (include/walkgpt_hip.h)


def _nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float, what: str) -> torch.Tensor:
    if boxes.shape[0] > NMS_MAX_BOXES:
        raise RuntimeError("SamAutomaticMaskGenerator: %d masks reach the NMS %s, the device NMS takes at most %d per call; raise pred_iou_thresh / "
                           "stability_score_thresh, or use fewer points or crop layers" % (boxes.shape[0], what, NMS_MAX_BOXES))
    return ops.nms(boxes, scores, iou_threshold)


def _box_area(boxes: torch.Tensor) -> torch.Tensor:
    """torchvision.ops.box_area: (x2 - x1) (y2 - y1), no +1."""
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def _empty(device) -> Dict[str, Any]:
    return {"rles": [], "iou_preds": torch.empty(0, device=device), "points": torch.empty(0, 2, dtype=torch.float64),
            "stability_score": torch.empty(0, device=device), "boxes": torch.empty(0, 4, dtype=torch.int32, device=device),
            "crop_boxes": torch.empty(0, 4, dtype=torch.int64)}


def _cat(parts: List[Dict[str, Any]], device) -> Dict[str, Any]:
    """MaskData.cat (amg.py:59-70) over a list of parts."""
    if not parts:
        return _empty(device)
    out = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0] if k != "rles"}
    out["rles"] = [r for p in parts for r in p["rles"]]
    return out


def _filter(data: Dict[str, Any], keep: torch.Tensor) -> Dict[str, Any]:
    """MaskData.filter (amg.py:44-57) with an index tensor."""
    idx = keep.cpu()
    out = {k: v[keep.to(v.device)] for k, v in data.items() if k != "rles"}
    out["rles"] = [data["rles"][i] for i in idx.tolist()]
    return out


class SamAutomaticMaskGenerator:
    def __init__(self, model: Sam, points_per_side: Optional[int] = 32, points_per_batch: int = 64, pred_iou_thresh: float = 0.88,
                 stability_score_thresh: float = 0.95, stability_score_offset: float = 1.0, box_nms_thresh: float = 0.7, crop_n_layers: int = 0,
                 crop_nms_thresh: float = 0.7, crop_overlap_ratio: float = 512 / 1500, crop_n_points_downscale_factor: int = 1,
                 point_grids: Optional[List[np.ndarray]] = None, min_mask_region_area: int = 0, output_mode: str = "binary_mask") -> None:
        """automatic_mask_generator.py:25-124; the arguments mean what they mean there.  min_mask_region_area > 0 uses scipy.ndimage where the
        reference uses OpenCV; output_mode "coco_rle" needs pycocotools, as in the reference (that branch is not covered by a test: pycocotools
        is not among this project's dependencies)."""
        assert (points_per_side is None) != (point_grids is None), "Exactly one of points_per_side or point_grid must be provided."
        if points_per_side is not None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers, crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert output_mode in ["binary_mask", "uncompressed_rle", "coco_rle"], f"Unknown output_mode {output_mode}."
        if output_mode == "coco_rle":
            from pycocotools import mask as mask_utils  # type: ignore # noqa: F401
        if min_mask_region_area > 0:
            from scipy import ndimage  # noqa: F401
        self.predictor = SamPredictor(model)
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode

    @torch.no_grad()
    def generate(self, image: np.ndarray) -> List[Dict[str, Any]]:
        """image HWC uint8 -> the records of automatic_mask_generator.py:127-187: segmentation (bool HW array, or the RLE dict), area, bbox XYWH,
        predicted_iou, point_coords, stability_score, crop_box XYWH."""
        if self.predictor.device.type != "cuda":
            raise RuntimeError("SamAutomaticMaskGenerator runs on the HIP path only (the model is on %s): move it to the GPU -- there is no CPU "
                               "fallback" % self.predictor.device)
        data = self._generate_masks(image)
        if self.min_mask_region_area > 0:
            data = self.postprocess_small_regions(data, self.min_mask_region_area, max(self.box_nms_thresh, self.crop_nms_thresh),
                                                  device=self.predictor.device)
        if self.output_mode == "coco_rle":
            segs = [coco_encode_rle(r) for r in data["rles"]]
        elif self.output_mode == "binary_mask":
            segs = [rle_to_mask(r) for r in data["rles"]]
        else:
            segs = data["rles"]
        return [{"segmentation": segs[i],
                 "area": area_from_rle(data["rles"][i]),
                 "bbox": box_xyxy_to_xywh(data["boxes"][i]).tolist(),
                 "predicted_iou": data["iou_preds"][i].item(),
                 "point_coords": [data["points"][i].tolist()],
                 "stability_score": data["stability_score"][i].item(),
                 "crop_box": box_xyxy_to_xywh(data["crop_boxes"][i]).tolist()} for i in range(len(segs))]

    def _generate_masks(self, image: np.ndarray) -> Dict[str, Any]:
        """automatic_mask_generator.py:189-215."""
        orig_size = image.shape[:2]
        crop_boxes, layer_idxs = generate_crop_boxes(orig_size, self.crop_n_layers, self.crop_overlap_ratio)
        dev = self.predictor.device
        data = _cat([self._process_crop(image, box, layer, orig_size) for box, layer in zip(crop_boxes, layer_idxs)], dev)
        if len(crop_boxes) > 1 and len(data["rles"]) > 0:
            # masks from smaller crops win (:203-212); equal scores inside a crop keep their order (the stable sort of ops.nms)
            scores = 1 / _box_area(data["crop_boxes"])
            data = _filter(data, _nms(data["boxes"].float(), scores.to(dev), self.crop_nms_thresh, "across crops"))
        out = {k: data[k].detach().cpu().numpy() for k in _KEYS}          # MaskData.to_numpy, amg.py:72-75
        out["rles"] = data["rles"]
        return out

    def _process_crop(self, image: np.ndarray, crop_box: List[int], crop_layer_idx: int, orig_size: Tuple[int, ...]) -> Dict[str, Any]:
        """automatic_mask_generator.py:217-258."""
        x0, y0, x1, y1 = crop_box
        cropped = image[y0:y1, x0:x1, :]
        size = cropped.shape[:2]
        self.predictor.set_image(cropped)
        points_for_image = self.point_grids[crop_layer_idx] * np.array(size)[None, ::-1]
        dev = self.predictor.device
        data = _cat([self._process_batch(points, size, crop_box, orig_size) for (points,) in batch_iterator(self.points_per_batch, points_for_image)],
                    dev)
        self.predictor.reset_image()
        if len(data["rles"]) > 0:
            data = _filter(data, _nms(data["boxes"].float(), data["iou_preds"], self.box_nms_thresh, "of one crop"))
        data["boxes"] = uncrop_boxes_xyxy(data["boxes"], crop_box)
        data["points"] = uncrop_points(data["points"], crop_box)
        data["crop_boxes"] = torch.tensor([crop_box for _ in range(len(data["rles"]))], dtype=torch.int64).reshape(-1, 4)
        return data

    def _process_batch(self, points: np.ndarray, im_size: Tuple[int, ...], crop_box: List[int], orig_size: Tuple[int, ...]) -> Dict[str, Any]:
        """automatic_mask_generator.py:260-321 without a full-resolution tensor."""
        orig_h, orig_w = orig_size
        pred = self.predictor
        dev = pred.device
        # apply_coords gives float64; the reference's prompt encoder adds 0.5 in double and only then casts to fp32 (prompt_encoder.py:80-82
        # on a float64 tensor).  The kernel adds its 0.5 in fp32, so it is handed fl32(p + 0.5) - 0.5: that difference is exact in fp32
        # (both operands are multiples of the result's last place), and adding 0.5 back returns fl32(p + 0.5) bit for bit.
        shifted = torch.as_tensor(pred.transform.apply_coords(points, im_size), dtype=torch.float64) + 0.5
        in_points = (shifted.to(torch.float32) - 0.5).to(dev)
        in_labels = torch.ones(in_points.shape[0], dtype=torch.int, device=dev)
        low_res, iou_preds = pred._predict_low_res(in_points[:, None, :], in_labels[:, None], None, None, True)
        n_per_point = low_res.shape[1]
        thr = pred.model.mask_threshold
        stats, bits = ops.amg_mask_stats(low_res.float().flatten(0, 1).contiguous(), pred.model.image_encoder.img_size, pred.input_size,
                                         pred.original_size, thr, self.stability_score_offset)
        iou_preds = iou_preds.flatten(0, 1)
        # the reference's filters in its order (:290-314), each on the [N, 8] tensor.  int32 / int32 is torch's true division: fp32, 0 / 0 = NaN,
        # which fails `>=` (calculate_stability_score, amg.py:176)
        stability = stats[:, 0] / stats[:, 1]
        keep = torch.ones_like(iou_preds, dtype=torch.bool)
        if self.pred_iou_thresh > 0.0:
            keep &= iou_preds > self.pred_iou_thresh
        if self.stability_score_thresh > 0.0:
            keep &= stability >= self.stability_score_thresh
        boxes = stats[:, 3:7]
        keep &= ~is_box_near_crop_edge(boxes, crop_box, [0, 0, orig_w, orig_h])
        idx = torch.nonzero(keep).reshape(-1)
        all_points = torch.as_tensor(points.repeat(n_per_point, axis=0))
        return {"rles": ops.amg_rle(bits, idx, crop_box, (orig_h, orig_w)), "iou_preds": iou_preds[idx], "points": all_points[idx.cpu()],
                "stability_score": stability[idx], "boxes": boxes[idx]}

    @staticmethod
    def postprocess_small_regions(mask_data: Dict[str, Any], min_area: int, nms_thresh: float, device=None) -> Dict[str, Any]:
        """automatic_mask_generator.py:323-372: fill small holes, drop small islands, NMS with score 0 for changed and 1 for unchanged masks, and
        re-encode only the changed survivors.  mask_data holds numpy arrays (after _generate_masks); the masks are decoded and re-encoded on
        the host (scipy.ndimage in place of OpenCV), the NMS is ops.nms on `device` (generate passes the model's; a direct caller who passes none
        gets the current device).  Host-only part without a reference fixture."""
        if len(mask_data["rles"]) == 0:
            return mask_data
        masks, scores = [], []
        for rle in mask_data["rles"]:
            mask, holes_changed = remove_small_regions(rle_to_mask(rle), min_area, mode="holes")
            mask, islands_changed = remove_small_regions(mask, min_area, mode="islands")
            masks.append(mask)
            scores.append(float(not (holes_changed or islands_changed)))
        boxes = np.stack([mask_to_box_numpy(m) for m in masks])
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        keep = _nms(torch.as_tensor(boxes, dtype=torch.float32, device=dev), torch.as_tensor(scores, device=dev), nms_thresh,
                    "after the small-region clean-up").cpu().numpy()
        for i in keep.tolist():
            if scores[i] == 0.0:
                mask_data["rles"][i] = mask_to_rle_numpy(masks[i])
                mask_data["boxes"][i] = boxes[i]
        out = {k: mask_data[k][keep] for k in _KEYS}
        out["rles"] = [mask_data["rles"][i] for i in keep.tolist()]
        return out
