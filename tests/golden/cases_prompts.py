"""Point / box / mask prompt cases (tests/golden/make_golden_prompts.py writes prompts_<grid>.npz and predictor_<name>.npz from them).

The image embedding, text rows and decoder weights are the decoder cases' own (cases.DECODERS, cases.decoder_case_weights); the prompt-encoder
parameters the text path never reads (point_embeddings, not_a_point_embed, mask_downscaling) come from synth.param under their state_dict keys.
"""
import numpy as np
import torch

from tests.golden import cases
from walkgpt_amd import synth

GRIDS = ("g32", "g64")
B = 3   # prompts per case

PROMPT_EXTRA_SHAPES = dict(
    [("prompt_encoder.point_embeddings.%d.weight" % i, (1, 256)) for i in range(4)] + [
        ("prompt_encoder.not_a_point_embed.weight", (1, 256)),
        ("prompt_encoder.mask_downscaling.0.weight", (4, 1, 2, 2)), ("prompt_encoder.mask_downscaling.0.bias", (4,)),
        ("prompt_encoder.mask_downscaling.1.weight", (4,)), ("prompt_encoder.mask_downscaling.1.bias", (4,)),
        ("prompt_encoder.mask_downscaling.3.weight", (16, 4, 2, 2)), ("prompt_encoder.mask_downscaling.3.bias", (16,)),
        ("prompt_encoder.mask_downscaling.4.weight", (16,)), ("prompt_encoder.mask_downscaling.4.bias", (16,)),
        ("prompt_encoder.mask_downscaling.6.weight", (256, 16, 1, 1)), ("prompt_encoder.mask_downscaling.6.bias", (256,))])

# kind -> (point labels per prompt or None, box, text, mask).  Labels cover -1 (not a point), 0, 1 and 2 (kept as the bare positional term).
KINDS = {
    "points": ([[1, 0], [1, 1], [0, 1]], False, False, False),
    "points_box": ([[1, 0], [0, 1], [1, 1]], True, False, False),
    "box": (None, True, False, False),
    "labels": ([[-1, 0, 1, 2], [2, 1, 0, -1], [1, -1, 2, 0]], False, False, False),
    "points_text": ([[1], [0], [1]], False, True, False),
    "mask": (None, False, False, True),
    "text_mask": (None, False, True, True),
}
# two-step refinement: step 1 = these points (single mask), step 2 = the same points + step 1's low-res logits as mask input
REFINE_LABELS = [[1], [1], [0]]


def prompt_weights(c):
    w = cases.decoder_case_weights(c)
    for k, sh in PROMPT_EXTRA_SHAPES.items():
        w[k] = torch.from_numpy(synth.param(c["seed"], k, sh))
    return w


def prompt_inputs(c, kind):
    """(coords [B,N,2] fp32 or None, labels [B,N] int32 or None, boxes [B,4] fp32 or None, text [B,1,256] fp32 or None, masks [B,1,4g,4g] fp32
    or None) in the input frame (S = 16 g pixels)."""
    labels, box, text, mask = KINDS[kind] if kind in KINDS else (REFINE_LABELS, False, False, False)
    g = c["grid"]
    S = 16 * g
    coords = lab = boxes = t = m = None
    if labels is not None:
        lab = torch.tensor(labels, dtype=torch.int32)
        coords = torch.from_numpy((synth.uniform01(c["seed"], "input.%s.coords" % kind, lab.numel() * 2) * S).astype(np.float32)).reshape(B, -1, 2)
    if box:
        u = (synth.uniform01(c["seed"], "input.%s.boxes" % kind, B * 4) * S).astype(np.float32).reshape(B, 2, 2)
        boxes = torch.from_numpy(np.concatenate([u.min(1), u.max(1)], 1))                   # x1 <= x2, y1 <= y2
    if text:
        t = cases.decoder_inputs(c)[1]
        t = t[torch.arange(B) % t.shape[0]].contiguous()                                       # (g64 has two text rows)
    if mask:
        m = torch.from_numpy(synth.normal(c["seed"], "input.%s.masks" % kind, (B, 1, 4 * g, 4 * g), 4.0))
    return coords, lab, boxes, t, m


def tap_dense(d):
    """[B, 256, g, g] dense embedding -> strided slice."""
    return d[:, ::8, ::4, ::4].contiguous()


def tap_masks(m):
    """[B, k, 4g, 4g] low-res logits -> [B, k, 32, 32]."""
    s = m.shape[-1] // 32
    return m[:, :, ::s, ::s].contiguous()


# ---- end to end through SamPredictor -------------------------------------------------------------------------------------------------------
PREDICTORS = {
    "b128": dict(seed=61, embed_dim=128, depth=1, heads=2, global_idx=[0], image_size=512, frame=(300, 420),
                 point=[[265.0, 140.0]], label=[1], box=[120.0, 60.0, 330.0, 250.0]),
}


def predictor_state_dict(c, model):
    """synth.param for every key of a Sam state_dict (the reference's names)."""
    return {k: torch.from_numpy(synth.param(c["seed"], k, tuple(v.shape))) for k, v in model.state_dict().items()}


def predictor_frame(c):
    h, w = c["frame"]
    u = synth.uniform01(c["seed"], "input.frame", h * w * 3).reshape(h, w, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = 0.45 * h, 0.6 * w
    blob = ((yy - cy) ** 2 / (0.3 * h) ** 2 + (xx - cx) ** 2 / (0.25 * w) ** 2 < 1.0)[..., None]
    base = np.where(blob, [200.0, 60.0, 50.0], [40.0, 110.0, 170.0])
    return np.clip(base + 30.0 * (u - 0.5) + 20.0 * np.sin(xx[..., None] / 19.0 + np.arange(3)), 0, 255).astype(np.uint8)
