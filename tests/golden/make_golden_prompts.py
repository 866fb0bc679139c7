"""Generate tests/golden/prompts_<grid>.npz and predictor_<name>.npz from the REFERENCE's own PromptEncoder, MaskDecoder, Sam and SamPredictor
(imported from the reference checkout through make_golden._import_reference) on the cases of cases_prompts.py, on CPU in fp32, plus the same
modules cast to bf16 as a calibration.  Only outputs (or strided taps of them) are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prompts.py [prompts] [predictor]

The reference's PromptEncoder.forward takes `text_embeds` as a required positional argument, so its own Sam.forward and
SamPredictor.predict_torch (which do not pass it) raise TypeError as written; the predictor case binds text_embeds=None on the instance.
"""
import importlib
import os
import sys
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tests.golden import cases, cases_prompts as cp  # noqa: E402
from tests.golden.make_golden import _import_reference  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _build(sam_modeling, c, w):
    g = c["grid"]
    pe = sam_modeling.PromptEncoder(embed_dim=256, image_embedding_size=(g, g), input_image_size=(g * 16, g * 16), mask_in_chans=16)
    dec = sam_modeling.MaskDecoder(num_multimask_outputs=3, transformer=sam_modeling.TwoWayTransformer(
        depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8), transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    for mod, prefix in ((pe, "prompt_encoder."), (dec, "mask_decoder.")):
        mod.load_state_dict({k: w[prefix + k] for k in mod.state_dict()}, strict=True)
        mod.eval()
    return pe, dec


def make_prompts(name):
    sam_modeling, _ = _import_reference()
    c = cases.DECODERS[name]
    w = cp.prompt_weights(c)
    pe, dec = _build(sam_modeling, c, w)
    pe16, dec16 = _build(sam_modeling, c, w)
    pe16.bfloat16()
    dec16.bfloat16()
    pe16.pe_layer.positional_encoding_gaussian_matrix.data = pe.pe_layer.positional_encoding_gaussian_matrix.data.clone()   # fp32, as in the build
    emb = cases.decoder_inputs(c)[0]
    out = {}

    def run(kind, coords, labels, boxes, text, masks, bf16=False):
        p, d = (pe16, dec16) if bf16 else (pe, dec)
        dt = torch.bfloat16 if bf16 else torch.float32
        pts = None if coords is None else (coords, labels)
        sparse, dense = p(points=pts, boxes=boxes, masks=None if masks is None else masks.to(dt),
                          text_embeds=None if text is None else text.to(dt))
        r = {"sparse": sparse.float(), "dense": dense.float()}
        for k, mm in (("1", False), ("3", True)):
            m, i = d(image_embeddings=emb.to(dt), image_pe=p.get_dense_pe().to(dt), sparse_prompt_embeddings=sparse.to(dt),
                     dense_prompt_embeddings=dense.to(dt), multimask_output=mm)
            r["masks" + k], r["iou" + k] = m.float(), i.float()
        return r

    with torch.no_grad():
        for kind in list(cp.KINDS) + ["refine"]:
            coords, labels, boxes, text, masks = cp.prompt_inputs(c, kind)
            if kind == "refine":
                step1 = run(kind, coords, labels, None, None, None)
                step1_16 = run(kind, coords, labels, None, None, None, bf16=True)
                out["refine_step1_masks1"] = cp.tap_masks(step1["masks1"]).numpy()
                r = run(kind, coords, labels, None, None, step1["masks1"])
                r16 = run(kind, coords, labels, None, None, step1_16["masks1"], bf16=True)
            else:
                r = run(kind, coords, labels, boxes, text, masks)
                r16 = run(kind, coords, labels, boxes, text, masks, bf16=True)
            out[kind + "_sparse"] = r["sparse"].numpy()
            if masks is not None or kind == "refine":
                out[kind + "_dense"] = cp.tap_dense(r["dense"]).numpy()
                out[kind + "_dense_bf16"] = cp.tap_dense(r16["dense"]).numpy()
            for k in ("1", "3"):
                out["%s_masks%s" % (kind, k)] = cp.tap_masks(r["masks" + k]).numpy()
                out["%s_iou%s" % (kind, k)] = r["iou" + k].numpy()
                out["%s_cal_masks%s" % (kind, k)] = np.float32(_rel(r16["masks" + k].numpy(), r["masks" + k].numpy()))
            print("  %s %s: sparse %s, reference bf16 vs fp32 rel L2: masks1 %.4f masks3 %.4f%s" % (
                name, kind, tuple(r["sparse"].shape), out[kind + "_cal_masks1"], out[kind + "_cal_masks3"],
                (", dense %.4f" % _rel(r16["dense"].numpy(), r["dense"].numpy())) if kind + "_dense" in out else ""))
    np.savez_compressed(os.path.join(HERE, "prompts_%s.npz" % name), **out)


def make_predictor(name):
    from PIL import Image
    sam_modeling, _ = _import_reference()
    tvf = sys.modules["torchvision.transforms.functional"]
    tvf.to_pil_image = lambda a: Image.fromarray(a)
    tvf.resize = lambda im, size: im.resize((size[1], size[0]), Image.BILINEAR)   # torchvision's resize of a PIL image
    tr = importlib.import_module("model.segment_anything.utils.transforms")
    tr.to_pil_image, tr.resize = tvf.to_pil_image, tvf.resize
    predictor_mod = importlib.import_module("model.segment_anything.predictor")
    c = cp.PREDICTORS[name]
    S = c["image_size"]
    g = S // 16

    def build():
        sam = sam_modeling.Sam(
            image_encoder=sam_modeling.ImageEncoderViT(depth=c["depth"], embed_dim=c["embed_dim"], img_size=S, mlp_ratio=4,
                                                       norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_heads=c["heads"], patch_size=16,
                                                       qkv_bias=True, use_rel_pos=True, global_attn_indexes=c["global_idx"], window_size=14,
                                                       out_chans=256),
            prompt_encoder=sam_modeling.PromptEncoder(embed_dim=256, image_embedding_size=(g, g), input_image_size=(S, S), mask_in_chans=16),
            mask_decoder=sam_modeling.MaskDecoder(num_multimask_outputs=3, transformer=sam_modeling.TwoWayTransformer(
                depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8), transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256))
        sam.load_state_dict(cp.predictor_state_dict(c, sam), strict=True)
        sam.eval()
        fwd = sam.prompt_encoder.forward
        sam.prompt_encoder.forward = lambda points, boxes, masks, text_embeds=None: fwd(points, boxes, masks, text_embeds)
        return sam

    frame = cp.predictor_frame(c)
    pt, lab, box = np.array(c["point"]), np.array(c["label"]), np.array(c["box"])
    with torch.no_grad():
        pred = predictor_mod.SamPredictor(build())
        pred.set_image(frame)
        masks, iou, low = pred.predict(point_coords=pt, point_labels=lab, box=box, multimask_output=True)
        # the same modules in bf16 (the PE matrix and the pixel statistics stay fp32, as in the build)
        sam16 = build()
        sam16.bfloat16()
        for b in ("pixel_mean", "pixel_std"):
            getattr(sam16, b).data = getattr(pred.model, b).data.clone()
        sam16.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data = \
            pred.model.prompt_encoder.pe_layer.positional_encoding_gaussian_matrix.data.clone()
        x = torch.as_tensor(pred.transform.apply_image(frame)).permute(2, 0, 1).contiguous()[None]
        feats = sam16.image_encoder(sam16.preprocess(x).bfloat16())
        sp, de = sam16.prompt_encoder(points=(torch.as_tensor(pred.transform.apply_coords(pt, frame.shape[:2]), dtype=torch.float)[None],
                                              torch.as_tensor(lab, dtype=torch.int)[None]),
                                      boxes=torch.as_tensor(pred.transform.apply_boxes(box, frame.shape[:2]), dtype=torch.float), masks=None)
        low16, iou16 = sam16.mask_decoder(image_embeddings=feats, image_pe=sam16.prompt_encoder.get_dense_pe().bfloat16(),
                                          sparse_prompt_embeddings=sp.bfloat16(), dense_prompt_embeddings=de, multimask_output=True)
        masks16 = sam16.postprocess_masks(low16.float(), tuple(x.shape[-2:]), frame.shape[:2])[0] > 0
    low16 = low16[0].float().numpy()
    inter = np.logical_and(masks, masks16.numpy()).sum((1, 2))
    union = np.logical_or(masks, masks16.numpy()).sum((1, 2))
    out = dict(low_res=low, iou=iou, masks_packed=np.packbits(masks), masks_shape=np.array(masks.shape), low_res_bf16=low16,
               iou_bf16=iou16[0].float().numpy(), cal_low_res=np.float32(_rel(low16, low)), cal_mask_iou=(inter / np.maximum(union, 1)).astype(np.float32))
    print("  predictor %s: masks %s (positive %.3f), iou %s; reference bf16 vs fp32: low-res rel L2 %.4f, mask IoU %s" % (
        name, masks.shape, masks.mean(), iou, out["cal_low_res"], out["cal_mask_iou"]))
    np.savez_compressed(os.path.join(HERE, "predictor_%s.npz" % name), **out)


if __name__ == "__main__":
    want = sys.argv[1:]
    torch.set_num_threads(8)
    for kind, fn, table in (("prompts", make_prompts, cp.GRIDS), ("predictor", make_predictor, cp.PREDICTORS)):
        if want and kind not in want:
            continue
        for name in table:
            print("generating %s:%s" % (kind, name), flush=True)
            fn(name)
