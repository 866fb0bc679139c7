"""SamPredictor.predict_torch latency at ViT-B / 1024 for point, box and mask-refinement prompts (1 and 64 prompts per call), timed with device
events after warm-up, plus the bytes the mask-prompt kernel moves.  Synthetic weights (walkgpt_amd.synth); prints one JSON line.

    python tools/bench_prompts.py [--iters 50] [--warmup 10]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_prompts.py --iters 20`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from walkgpt_amd import synth  # noqa: E402
from walkgpt_amd.segment_anything import SamPredictor, build_sam_vit_b  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sam = build_sam_vit_b()
    sd = {k: torch.from_numpy(synth.param(7, k, tuple(v.shape))) for k, v in sam.state_dict().items()}
    sam.load_state_dict(sd, strict=True)
    G = sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data.clone()
    mean, std = sam.pixel_mean.data.clone(), sam.pixel_std.data.clone()
    sam.to(dev).bfloat16()
    sam.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data = G.to(dev)
    sam.pixel_mean.data, sam.pixel_std.data = mean.to(dev), std.to(dev)
    pred = SamPredictor(sam)
    u = synth.uniform01(7, "bench.frame", 720 * 960 * 3).reshape(720, 960, 3)
    pred.set_image((u * 255).astype(np.uint8))
    torch.cuda.synchronize()
    S = 1024
    res = {}
    for P in (1, 64):
        g = torch.Generator().manual_seed(P)
        pts = (torch.rand(P, 1, 2, generator=g) * 700).to(dev)
        lab = torch.ones(P, 1, dtype=torch.int32, device=dev)
        xy = torch.rand(P, 2, generator=g) * 500
        box = torch.cat([xy, xy + 200], 1).to(dev)
        mask = torch.randn(P, 1, 256, 256, generator=g).to(dev)
        calls = {"point": lambda: pred.predict_torch(pts, lab, multimask_output=True),
                 "box": lambda: pred.predict_torch(None, None, boxes=box, multimask_output=False),
                 "mask_refine": lambda: pred.predict_torch(pts, lab, mask_input=mask, multimask_output=False)}
        for name, fn in calls.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res["%s_p%d_ms" % (name, P)] = round(e0.elapsed_time(e1) / a.iters, 4)
    # wg_mask_embed_bf16 traffic per call: fp32 masks in, bf16 [P, 64*64, 256] rows out (weights: 18 KB, cached)
    res["mask_embed_bytes_p64"] = 64 * (256 * 256 * 4 + 64 * 64 * 256 * 2)
    res["mask_embed_bytes_p1"] = 256 * 256 * 4 + 64 * 64 * 256 * 2
    print(json.dumps(res))


if __name__ == "__main__":
    main()
