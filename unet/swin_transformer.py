"""Dotted-path alias so `unet.swin_transformer.swin_b` resolves to the HIP implementation."""
from adm_amd.unet.swin_transformer import *  # noqa: F401,F403
from adm_amd.unet.swin_transformer import SwinTransformer, load_encoder_weights, swin_b  # noqa: F401
