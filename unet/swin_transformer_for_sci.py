"""Dotted-path alias so `unet.swin_transformer_for_sci.swin_b` resolves to the HIP implementation (one-channel stem)."""
from adm_amd.unet.swin_transformer_for_sci import SwinTransformer, load_encoder_weights, swin_b  # noqa: F401
