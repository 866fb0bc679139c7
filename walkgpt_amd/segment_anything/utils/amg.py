"""Host logic of the reference's model/segment_anything/utils/amg.py that SamAutomaticMaskGenerator needs.

What the reference does here on full-resolution tensors (calculate_stability_score :156-176, batched_mask_to_box :303-346, uncrop_masks :255-264,
mask_to_rle_pytorch :107-135) is wg_amg_mask_stats_f32 / wg_amg_rle_*_i32 on this path (walkgpt_amd.ops); this module keeps the small-tensor and
numpy pieces: point grids, crop boxes, the crop-edge filter, RLE decoding and the small-region clean-up.
"""
import math
from typing import Any, Dict, List, Tuple

import numpy as np
import torch


def build_point_grid(n_per_side: int) -> np.ndarray:
    """amg.py:179-186: n x n points at the cell centres of [0, 1]^2, (x, y) rows, x fastest."""
    half = 1 / (2 * n_per_side)
    side = np.linspace(half, 1 - half, n_per_side)
    xs, ys = np.tile(side[None, :], (n_per_side, 1)), np.tile(side[:, None], (1, n_per_side))
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side: int, n_layers: int, scale_per_layer: int) -> List[np.ndarray]:
    """amg.py:189-197: one grid per crop layer, int(n / scale**layer) points per side."""
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size: Tuple[int, ...], n_layers: int, overlap_ratio: float) -> Tuple[List[List[int]], List[int]]:
    """amg.py:200-234: the whole frame, then (2**i)**2 overlapping XYXY crops for layer i; returns (boxes, layer index of each)."""
    im_h, im_w = im_size
    boxes, layers = [[0, 0, im_w, im_h]], [0]
    short = min(im_h, im_w)
    for layer in range(n_layers):
        per_side = 2 ** (layer + 1)
        overlap = int(overlap_ratio * short * (2 / per_side))
        crop_w = int(math.ceil((overlap * (per_side - 1) + im_w) / per_side))
        crop_h = int(math.ceil((overlap * (per_side - 1) + im_h) / per_side))
        for i in range(per_side):                      # (x outer, y inner: itertools.product(x0s, y0s), amg.py:229)
            x0 = int((crop_w - overlap) * i)
            for j in range(per_side):
                y0 = int((crop_h - overlap) * j)
                boxes.append([x0, y0, min(x0 + crop_w, im_w), min(y0 + crop_h, im_h)])
                layers.append(layer + 1)
    return boxes, layers


def batch_iterator(batch_size: int, *args):
    """amg.py:98-104."""
    assert len(args) > 0 and all(len(a) == len(args[0]) for a in args), "Batched iteration must have inputs of all the same size."
    for b in range(0, len(args[0]), batch_size):
        yield [a[b:b + batch_size] for a in args]


def uncrop_boxes_xyxy(boxes: torch.Tensor, crop_box: List[int]) -> torch.Tensor:
    """amg.py:237-243."""
    x0, y0 = crop_box[0], crop_box[1]
    return boxes + torch.tensor([[x0, y0, x0, y0]], device=boxes.device)


def uncrop_points(points: torch.Tensor, crop_box: List[int]) -> torch.Tensor:
    """amg.py:246-252."""
    return points + torch.tensor([[crop_box[0], crop_box[1]]], device=points.device)


def is_box_near_crop_edge(boxes: torch.Tensor, crop_box: List[int], orig_box: List[int], atol: float = 20.0) -> torch.Tensor:
    """amg.py:78-88: a side of the (crop-frame) box within atol of the crop's side, unless that is the frame's own side."""
    crop = torch.as_tensor(crop_box, dtype=torch.float, device=boxes.device)[None, :]
    orig = torch.as_tensor(orig_box, dtype=torch.float, device=boxes.device)[None, :]
    b = uncrop_boxes_xyxy(boxes, crop_box).float()
    near_crop = torch.isclose(b, crop, atol=atol, rtol=0)
    near_frame = torch.isclose(b, orig, atol=atol, rtol=0)
    return torch.any(near_crop & ~near_frame, dim=1)


def box_xyxy_to_xywh(box):
    """amg.py:91-95 (a copy; the input stays)."""
    out = box.copy() if isinstance(box, np.ndarray) else box.clone()
    out[2] = out[2] - out[0]
    out[3] = out[3] - out[1]
    return out


def area_from_rle(rle: Dict[str, Any]) -> int:
    """amg.py:152-153."""
    return int(sum(rle["counts"][1::2]))


def rle_to_mask(rle: Dict[str, Any]) -> np.ndarray:
    """amg.py:138-149, with np.repeat over the runs instead of a Python loop per run: bool [H, W]."""
    h, w = rle["size"]
    counts = np.asarray(rle["counts"], dtype=np.int64)
    flat = np.repeat(np.arange(counts.size) & 1, counts).astype(bool)
    return flat.reshape(w, h).transpose()


def mask_to_rle_numpy(mask: np.ndarray) -> Dict[str, Any]:
    """mask_to_rle_pytorch (amg.py:107-135) of ONE bool [H, W] mask that is already on the host (postprocess_small_regions)."""
    h, w = mask.shape
    flat = np.asarray(mask, dtype=bool).transpose().reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate([[0], change, [h * w]])).tolist()
    return {"size": [h, w], "counts": ([0] + runs) if flat[0] else runs}


def mask_to_box_numpy(mask: np.ndarray) -> np.ndarray:
    """batched_mask_to_box (amg.py:303-346) of one bool [H, W] mask: XYXY in inclusive pixel indices, zeros when empty."""
    ys, xs = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
    if ys.size == 0:
        return np.zeros(4, dtype=np.int64)
    return np.array([xs[0], ys[0], xs[-1], ys[-1]], dtype=np.int64)


def remove_small_regions(mask: np.ndarray, area_thresh: float, mode: str) -> Tuple[np.ndarray, bool]:
    """amg.py:267-291 on scipy.ndimage.label with the 8-connected structure in place of cv2.connectedComponentsWithStats(.., 8): fills holes
    (mode "holes") or drops islands (mode "islands") smaller than area_thresh; if every island is small the largest stays.  Returns (mask,
    changed).  Host-only, and there is no reference fixture for it: the reference's version needs OpenCV, which the fixtures' maker does not
    have; tests/test_amg_host.py checks it on hand-made masks."""
    from scipy import ndimage
    assert mode in ["holes", "islands"]
    holes = mode == "holes"
    work = np.logical_xor(holes, mask)
    regions, n = ndimage.label(work, structure=np.ones((3, 3), dtype=bool))
    sizes = np.bincount(regions.reshape(-1), minlength=n + 1)[1:]          # label 0 is the background
    small = [i + 1 for i, s in enumerate(sizes) if s < area_thresh]
    if len(small) == 0:
        return mask, False
    fill = [0] + small
    if not holes:
        fill = [i for i in range(n + 1) if i not in fill]
        if len(fill) == 0:
            fill = [int(np.argmax(sizes)) + 1]
    return np.isin(regions, fill), True


def coco_encode_rle(uncompressed_rle: Dict[str, Any]) -> Dict[str, Any]:
    """amg.py:294-300 (needs pycocotools)."""
    from pycocotools import mask as mask_utils  # type: ignore
    h, w = uncompressed_rle["size"]
    rle = mask_utils.frPyObjects(uncompressed_rle, h, w)
    rle["counts"] = rle["counts"].decode("utf-8")
    return rle
