"""SamPredictor of the reference (model/segment_anything/predictor.py) on the HIP path.

Same methods, arguments, attributes and return values.  set_image uploads the uint8 frame and runs Pillow's resize, the normalisation and
the padding as one kernel (walkgpt_amd.preprocess.preprocess_frames with SAM's pixel mean / std), then the image encoder; predict /
predict_torch run the prompt encoder (wg_prompt_sparse_f32, wg_mask_embed_bf16), the mask decoder and the fused postprocess.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from ..preprocess import ResizeLongestSide, preprocess_frames
from .modeling import Sam


class SamPredictor:
    def __init__(self, sam_model: Sam) -> None:
        self.model = sam_model
        self.transform = ResizeLongestSide(sam_model.image_encoder.img_size)
        self.reset_image()

    def set_image(self, image: np.ndarray, image_format: str = "RGB") -> None:
        """image: HWC uint8 in [0, 255], RGB or BGR."""
        assert image_format in ["RGB", "BGR"], f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        if image_format != self.model.image_format:
            image = image[..., ::-1]
        frame = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)).to(self.device)
        mean = tuple(float(v) for v in self.model.pixel_mean.float().reshape(-1).tolist())
        std = tuple(float(v) for v in self.model.pixel_std.float().reshape(-1).tolist())
        with torch.no_grad():
            x, _, input_size = preprocess_frames(frame[None], self.model.image_encoder.img_size, mean, std)
            self._set_features(x, input_size, image.shape[:2])

    @torch.no_grad()
    def set_torch_image(self, transformed_image: torch.Tensor, original_image_size: Tuple[int, ...]) -> None:
        """transformed_image: 1x3xHxW, already resized with ResizeLongestSide (long side == img_size)."""
        assert (len(transformed_image.shape) == 4 and transformed_image.shape[1] == 3
                and max(*transformed_image.shape[2:]) == self.model.image_encoder.img_size), \
            f"set_torch_image input must be BCHW with long side {self.model.image_encoder.img_size}."
        self._set_features(self.model.preprocess(transformed_image), tuple(transformed_image.shape[-2:]), original_image_size)

    def _set_features(self, x, input_size, original_size):
        self.reset_image()
        self.original_size = tuple(int(v) for v in original_size)
        self.input_size = tuple(int(v) for v in input_size)
        self.features = self.model.image_encoder(x)
        self.is_image_set = True

    def predict(self, point_coords: Optional[np.ndarray] = None, point_labels: Optional[np.ndarray] = None, box: Optional[np.ndarray] = None,
                mask_input: Optional[np.ndarray] = None, multimask_output: bool = True,
                return_logits: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Prompts in the original frame's pixels (point_coords Nx2 (X, Y), point_labels N, box XYXY), mask_input 1x256x256 low-res logits
        -> (masks CxHxW, iou C, low-res logits Cx256x256) as numpy arrays."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        coords_torch, labels_torch, box_torch, mask_input_torch = None, None, None, None
        if point_coords is not None:
            assert point_labels is not None, "point_labels must be supplied if point_coords is supplied."
            point_coords = self.transform.apply_coords(point_coords, self.original_size)
            coords_torch = torch.as_tensor(point_coords, dtype=torch.float, device=self.device)[None, :, :]
            labels_torch = torch.as_tensor(point_labels, dtype=torch.int, device=self.device)[None, :]
        if box is not None:
            box = self.transform.apply_boxes(box, self.original_size)
            box_torch = torch.as_tensor(box, dtype=torch.float, device=self.device)[None, :]
        if mask_input is not None:
            mask_input_torch = torch.as_tensor(mask_input, dtype=torch.float, device=self.device)[None, :, :, :]
        masks, iou_predictions, low_res_masks = self.predict_torch(coords_torch, labels_torch, box_torch, mask_input_torch, multimask_output,
                                                                   return_logits=return_logits)
        return masks[0].detach().cpu().numpy(), iou_predictions[0].detach().cpu().numpy(), low_res_masks[0].detach().cpu().numpy()

    @torch.no_grad()
    def predict_torch(self, point_coords: Optional[torch.Tensor], point_labels: Optional[torch.Tensor], boxes: Optional[torch.Tensor] = None,
                      mask_input: Optional[torch.Tensor] = None, multimask_output: bool = True,
                      return_logits: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Batched prompts already in the input frame (BxNx2, BxN, Bx4, Bx1x256x256) -> (masks BxCxHxW, iou BxC, low-res logits BxCx256x256)."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        low_res_masks, iou_predictions = self._predict_low_res(point_coords, point_labels, boxes, mask_input, multimask_output)
        masks = self.model.postprocess_masks(low_res_masks, self.input_size, self.original_size)
        if not return_logits:
            masks = masks > self.model.mask_threshold
        return masks, iou_predictions, low_res_masks

    @torch.no_grad()
    def _predict_low_res(self, point_coords, point_labels, boxes, mask_input, multimask_output):
        """predict_torch up to the decoder: (low-res logits BxCx256x256, iou BxC), nothing at the frame's size (SamAutomaticMaskGenerator
        takes its statistics straight from the low-res logits)."""
        points = (point_coords, point_labels) if point_coords is not None else None
        pe = self.model.prompt_encoder
        sparse, dense = pe(points=points, boxes=boxes, masks=mask_input)
        return self.model.mask_decoder(image_embeddings=self.features, image_pe=pe.get_dense_pe(), sparse_prompt_embeddings=sparse,
                                       dense_prompt_embeddings=dense, multimask_output=multimask_output)

    def get_image_embedding(self) -> torch.Tensor:
        """The current image's embedding, 1xCxHxW."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        assert self.features is not None, "Features must exist if an image has been set."
        return self.features

    @property
    def device(self) -> torch.device:
        return self.model.device

    def reset_image(self) -> None:
        self.is_image_set = False
        self.features = None
        self.original_size = None
        self.input_size = None
        self.orig_h = None
        self.orig_w = None
        self.input_h = None
        self.input_w = None
