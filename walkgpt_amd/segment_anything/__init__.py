"""HIP-backed SAM modules with the reference's public names (model/segment_anything/__init__.py, build_sam.py, predictor.py,
automatic_mask_generator.py)."""
from .modeling import (ImageEncoderViT, MaskDecoder, PromptEncoder, Sam, TwoWayTransformer, build_sam,  # noqa: F401
                       build_sam_vit_b, build_sam_vit_h, build_sam_vit_l, sam_model_registry)
from .predictor import SamPredictor  # noqa: F401
from .automatic_mask_generator import SamAutomaticMaskGenerator  # noqa: F401
