"""SamAutomaticMaskGenerator cases (tests/golden/make_golden_amg.py writes amg_stats_<case>.npz, amg_host_h1.npz and amg_e2e_b128.npz from them).

Inputs are rebuilt from (seed, key) by walkgpt_amd.synth; the fixtures hold the reference's outputs only.
"""
import numpy as np

from walkgpt_amd import synth

THR, OFF = 0.0, 1.0          # Sam.mask_threshold and the generator's default stability_score_offset

# ---- mask statistics: (low-res side, padded image side, input size, output size) ---------------------------------------------------------------
# g3 has one row block of 32 plus one row, and a second column block of a single pixel.
STATS = {
    "g1": dict(seed=71, lh=64, img=256, input=(171, 256), output=(300, 450), n=70),
    "g2": dict(seed=72, lh=64, img=256, input=(256, 200), output=(97, 76), n=70),
    "g3": dict(seed=73, lh=32, img=128, input=(128, 128), output=(33, 257), n=70),
}
BAND_MAX = 0.002             # share of the frame's pixels within delta of a threshold, per mask and threshold (the maker asserts it)


def stats_delta(ref_abs_max):
    """The bound tests/test_gpu_misc.py::test_postprocess_and_score holds the HIP postprocess to against the reference."""
    return 1e-4 * ref_abs_max + 1e-5


def stats_logits(c, attempt=0):
    """fp32 [n, lh, lh] low-res logits: n - 3 masks of a smooth random field plus a blob that lies inside the valid part of the padded square
    (so the box lies inside the frame), then all below thr - off, all above thr + off, and a single low-res peak."""
    n, lh = c["n"], c["lh"]
    seed = c["seed"] + 1000 * attempt
    vy, vx = lh * c["input"][0] / c["img"], lh * c["input"][1] / c["img"]          # the valid rows / columns of the low-res square
    yy, xx = np.mgrid[0:lh, 0:lh].astype(np.float64)
    out = np.empty((n, lh, lh), dtype=np.float32)
    u = synth.uniform01(seed, "amg.stats.u", (n - 3) * 32).reshape(n - 3, 32)
    for i in range(n - 3):
        f = np.zeros((lh, lh))
        for k in range(5):                                                           # a few low-frequency waves: smooth, no plateau at a threshold
            fx, fy = 3.0 * (u[i, 4 * k] - 0.5), 3.0 * (u[i, 4 * k + 1] - 0.5)
            f += (0.3 + 0.5 * u[i, 4 * k + 2]) * np.sin(2 * np.pi * (fx * xx / vx + fy * yy / vy + u[i, 4 * k + 3]))
        cy, cx = (0.3 + 0.4 * u[i, 20]) * vy, (0.3 + 0.4 * u[i, 21]) * vx
        sy, sx = (0.08 + 0.12 * u[i, 22]) * vy, (0.08 + 0.12 * u[i, 23]) * vx
        blob = np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
        out[i] = (9.0 * blob - 4.0 + f).astype(np.float32)
    out[n - 3] = -3.0 + 0.5 * np.sin(xx / 5.0)                                       # empty at every threshold
    out[n - 2] = 3.0 + 0.5 * np.cos(yy / 7.0)                                        # full at every threshold
    out[n - 1] = -6.0
    out[n - 1, int(0.5 * vy), int(0.5 * vx)] = 30.0                                  # one low-res peak
    return out


# ---- host pieces ------------------------------------------------------------------------------------------------------------------------
HOST = dict(seed=81, grid=(4, 2, 2), frame=(300, 420), crop_layers=2, overlap=512 / 1500, rle_frame=(97, 76), rle_crop=(70, 45),
            rle_offsets=[(9, 13), (31, 27), (0, 0)],       # (x0, y0): inside the frame; touching its right and bottom sides; its first pixel
            nms_n=200, nms_thresholds=(0.3, 0.7))
EDGE_CROP, EDGE_ORIG = [100, 0, 320, 200], [0, 0, 420, 300]
# crop-frame XYXY boxes: clear of every side; within 20 px of the crop's left / right / bottom; at the top, which is the frame's own; on the limit
EDGE_BOXES = [[40, 40, 100, 100], [10, 50, 90, 120], [60, 30, 215, 90], [50, 60, 120, 190], [30, 0, 150, 60], [21, 30, 199, 179],
              [20, 30, 150, 100], [30, 30, 200, 100], [0, 0, 0, 0], [0, 0, 220, 200], [25, 5, 60, 179], [25, 5, 60, 181]]


def rle_patterns(h, w):
    """Six bool [h, w] masks: empty, full, first pixel, last pixel, a column ending in 1 followed by a column starting in 1, a checkerboard."""
    m = np.zeros((6, h, w), dtype=bool)
    m[1] = True
    m[2, 0, 0] = True
    m[3, h - 1, w - 1] = True
    m[4, h - 3:, 7] = True
    m[4, :5, 8] = True
    m[4, 20:40, 30] = True
    yy, xx = np.mgrid[0:h, 0:w]
    m[5] = (yy + xx) % 2 == 0
    return m


def pack_bits(masks):
    """bool [N, h, w] -> the kernels' layout, int32 [N, ceil(h / 32), w]: bit r of word (yb, x) = masks[n, 32 yb + r, x]."""
    n, h, w = masks.shape
    hb = (h + 31) // 32
    pad = np.zeros((n, hb * 32, w), dtype=np.uint64)
    pad[:, :h] = masks
    words = (pad.reshape(n, hb, 32, w) << np.arange(32, dtype=np.uint64)[None, None, :, None]).sum(2)
    return words.astype(np.uint32).view(np.int32)


def unpack_bits(bits, h):
    """the inverse: int32 [N, hb, w] -> bool [N, h, w]."""
    n, hb, w = bits.shape
    b = bits.view(np.uint32)[:, :, None, :] >> np.arange(32, dtype=np.uint32)[None, None, :, None]
    return (b & 1).astype(bool).reshape(n, hb * 32, w)[:, :h]


def positions_numpy(mask_in_frame):
    """Change positions of one bool [H, W] mask in the column-major flattening: every p >= 1 with bit[p] != bit[p - 1]."""
    flat = mask_in_frame.transpose().reshape(-1)
    return np.flatnonzero(flat[1:] != flat[:-1]) + 1


def place(mask, x0, y0, H, W):
    out = np.zeros((H, W), dtype=bool)
    out[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]] = mask
    return out


def nms_boxes(c=HOST):
    """(boxes fp32 [n, 4] XYXY, scores fp32 [n], tied scores fp32 [n] drawn from three values)."""
    n = c["nms_n"]
    u = synth.uniform01(c["seed"], "amg.nms", n * 6).reshape(n, 6)
    cx, cy = 300.0 * u[:, 0], 300.0 * u[:, 1]
    w, h = 10.0 + 110.0 * u[:, 2], 10.0 + 110.0 * u[:, 3]
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
    tied = np.array([0.25, 0.5, 1.0], dtype=np.float32)[(u[:, 5] * 3).astype(np.int64) % 3]
    return boxes, u[:, 4].astype(np.float32), tied


def pad_lists(lists, fill=-1):
    """list of int lists -> (int64 [n, longest] padded with `fill`, int64 [n] lengths)."""
    out = np.full((len(lists), max([len(v) for v in lists] + [1])), fill, dtype=np.int64)
    for i, v in enumerate(lists):
        out[i, :len(v)] = v
    return out, np.array([len(v) for v in lists], dtype=np.int64)


def unpad_lists(arr, lens):
    return [arr[i, :int(n)].tolist() for i, n in enumerate(lens)]


# ---- end to end: cases_prompts.PREDICTORS["b128"], its frame and weights ------------------------------------------------------------------------
# Random weights do not clear the generator's default thresholds; these come from the reference's own score distributions on this case (the maker
# prints them) so that between 8 and 64 records survive (the maker asserts that): predicted IoU runs from -0.97 to 0.52 with the median at -0.01,
# the logits seldom pass +1, so the stability score stays below 0.01 (three quarters below 0.0002), and the masks cover so much of the frame that
# their boxes nearly coincide -- at the default 0.7 either NMS leaves a single record, hence crop_nms_thresh is named as well.  All three score
# filters are live: both generators skip a filter whose threshold is not > 0, so pred_iou_thresh is positive (0.05 drops 60 % of the 192 masks of
# the whole-frame crop), and the stability threshold drops half of what is left.
E2E = dict(predictor="b128", points_per_side=8, points_per_batch=16, crop_n_layers=1, output_mode="uncompressed_rle",
           pred_iou_thresh=0.05, stability_score_thresh=0.00005, box_nms_thresh=0.998, crop_nms_thresh=0.998)
MATCH_IOU = 0.9              # two records match when they come from the same crop box and their masks' IoU is at least this


def e2e_kwargs(c=E2E):
    return {k: v for k, v in c.items() if k != "predictor"}


def rle_mask(size, counts):
    """bool [H, W] from an uncompressed RLE (column-major runs, starting with a 0 run)."""
    h, w = size
    counts = np.asarray(counts, dtype=np.int64)
    return np.repeat(np.arange(counts.size) & 1, counts).astype(bool).reshape(w, h).transpose()


def unmatched_share(records_a, records_b):
    """Share of records_a without a record of records_b from the same crop box whose mask IoU is >= MATCH_IOU; also the matched index pairs.
    A record here is (crop_box list, bool mask)."""
    pairs, miss = [], 0
    for i, (ca, ma) in enumerate(records_a):
        best, best_j = 0.0, -1
        for j, (cb, mb) in enumerate(records_b):
            if list(ca) != list(cb):
                continue
            union = np.logical_or(ma, mb).sum()
            iou = np.logical_and(ma, mb).sum() / union if union else 1.0
            if iou > best:
                best, best_j = iou, j
        if best >= MATCH_IOU:
            pairs.append((i, best_j))
        else:
            miss += 1
    return miss / max(len(records_a), 1), pairs
