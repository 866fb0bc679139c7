"""SamAutomaticMaskGenerator.generate at ViT-B / 1024 on a 1500 x 2250 frame with 32 x 32 points in batches of 64, and its three stages (image
encoder; prompt encoder + mask decoder; everything after the decoder), beside the plain composition of tests/amg_reference.py (full-resolution
logits from predict_torch, torch thresholds and boxes, numpy RLE, torch greedy NMS) in the same process.  Synthetic weights (walkgpt_amd.synth)
do not clear the default thresholds (their predicted IoU is mostly negative, and a pred_iou_thresh that is not > 0 switches that filter off
in the reference and here alike), so the predicted-IoU filter is off and the stability threshold is set from a calibration pass to the 2/3
quantile: roughly a third of the masks survive the filters.  The survivors are also counted inside a run of each path (the masks that reach the
run-length coding) and that count is what the JSON line reports.  Medians of repeated runs, timed on the host around device synchronisation; the stage times come from separate runs with
a synchronisation after each stage, the totals from runs without.  Prints one JSON line.

    python tools/bench_amg.py [--runs 5] [--ref-runs 3] [--points 32] [--frame 1500 2250]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import amg_reference as ar  # noqa: E402
from walkgpt_amd import ops, synth  # noqa: E402
from walkgpt_amd.segment_anything import SamAutomaticMaskGenerator, build_sam_vit_b  # noqa: E402


class Stages:
    """Wraps set_image and _predict_low_res of a predictor with synchronised timers."""

    def __init__(self, predictor):
        self.p, self.t = predictor, {"encoder": 0.0, "decoder": 0.0}
        self.saved = (predictor.set_image, predictor._predict_low_res)
        predictor.set_image = self._timed("encoder", self.saved[0])
        predictor._predict_low_res = self._timed("decoder", self.saved[1])

    def _timed(self, key, fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.t[key] += time.perf_counter() - t0
            return out
        return run

    def restore(self):
        self.p.set_image, self.p._predict_low_res = self.saved


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ref-runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frame", type=int, nargs=2, default=[1500, 2250])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sam = build_sam_vit_b()
    sam.load_state_dict({k: torch.from_numpy(synth.param(7, k, tuple(v.shape))) for k, v in sam.state_dict().items()}, strict=True)
    G = sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data.clone()
    mean, std = sam.pixel_mean.data.clone(), sam.pixel_std.data.clone()
    sam.to(dev).bfloat16()
    sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data = G.to(dev)
    sam.pixel_mean.data, sam.pixel_std.data = mean.to(dev), std.to(dev)
    H, W = a.frame
    frame = (synth.uniform01(7, "bench.amg.frame", H * W * 3).reshape(H, W, 3) * 255).astype(np.uint8)

    # calibration: the score distributions of every mask of the frame -> thresholds that keep about two thirds, then half of those
    gen = SamAutomaticMaskGenerator(sam, points_per_side=a.points, points_per_batch=a.batch, pred_iou_thresh=0.0, stability_score_thresh=0.0,
                                    output_mode="uncompressed_rle")
    pred = gen.predictor
    pred.set_image(frame)
    grid = gen.point_grids[0] * np.array([W, H])[None]
    iou, stab = [], []
    with torch.no_grad():
        for b in range(0, len(grid), a.batch):
            pts = torch.as_tensor(pred.transform.apply_coords(grid[b:b + a.batch], (H, W)), dtype=torch.float32, device=dev)
            low, i = pred._predict_low_res(pts[:, None], torch.ones(len(pts), 1, dtype=torch.int, device=dev), None, None, True)
            s, _ = ops.amg_mask_stats(low.float().flatten(0, 1).contiguous(), 1024, pred.input_size, pred.original_size, 0.0, 1.0)
            iou.append(i.flatten())
            stab.append(s[:, 0] / s[:, 1])
    iou, stab = torch.cat(iou).float(), torch.nan_to_num(torch.cat(stab), nan=0.0)
    iou_thr = 0.0                                                   # off: see the module docstring
    stab_thr = max(float(torch.quantile(stab, 2 / 3)), 1e-9)
    kw = dict(points_per_batch=a.batch, pred_iou_thresh=iou_thr, stability_score_thresh=stab_thr, box_nms_thresh=0.7, crop_n_layers=0,
              crop_nms_thresh=0.7)
    gen = SamAutomaticMaskGenerator(sam, points_per_side=a.points, output_mode="uncompressed_rle", **kw)

    def ours():
        return gen.generate(frame)

    def plain():
        return ar.generate(gen.predictor, frame, gen.point_grids, kw["points_per_batch"], iou_thr, stab_thr, 1.0, 0.7, 0, 0.7, 512 / 1500)

    # survivors = masks that reach the run-length coding, counted in the warm-up run of each path
    counted = {"fused": 0, "plain": 0}
    rle_fused, rle_plain = ops.amg_rle, ar.rle_numpy

    def count_fused(bits, keep, *rest):
        counted["fused"] += int(keep.shape[0])
        return rle_fused(bits, keep, *rest)

    def count_plain(mask):
        counted["plain"] += 1
        return rle_plain(mask)

    n_masks = 3 * a.points ** 2
    res = {"frame": [H, W], "masks": n_masks, "pred_iou_thresh": iou_thr, "stability_score_thresh": stab_thr,
           "predicted_iou_median": round(float(iou.median()), 4)}
    for name, fn, runs in (("fused", ours, a.runs), ("plain", plain, a.ref_runs)):
        ops.amg_rle, ar.rle_numpy = count_fused, count_plain
        try:
            _, out = timed(fn)                                         # warm-up, with the survivors counted
        finally:
            ops.amg_rle, ar.rle_numpy = rle_fused, rle_plain
        res[name + "_survivors"] = counted[name]
        res[name + "_surviving_share"] = round(counted[name] / n_masks, 3)
        res[name + "_records"] = len(out)
        res[name + "_total_ms"] = round(1e3 * statistics.median(timed(fn)[0] for _ in range(runs)), 2)
        enc, dec, post = [], [], []
        for _ in range(runs):
            st = Stages(gen.predictor)
            try:
                t, _ = timed(fn)
            finally:
                st.restore()
            enc.append(st.t["encoder"])
            dec.append(st.t["decoder"])
            post.append(t - st.t["encoder"] - st.t["decoder"])
        for k, v in (("encoder", enc), ("decoder", dec), ("post", post)):
            res["%s_%s_ms" % (name, k)] = round(1e3 * statistics.median(v), 2)
    res["post_ratio_plain_over_fused"] = round(res["plain_post_ms"] / res["fused_post_ms"], 2)
    res["total_ratio_plain_over_fused"] = round(res["plain_total_ms"] / res["fused_total_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
