"""The reference's import path of the single-channel condition encoder (/root/reference/unet/swin_transformer_for_sci.py).  That file
is swin_transformer.py with a one-channel patch embedding; here both are one module, and ``swin_b`` of this one defaults to
``in_chans=1``."""
from .swin_transformer import SwinTransformer, load_encoder_weights
from .swin_transformer import swin_b as _swin_b

__all__ = ["SwinTransformer", "swin_b", "load_encoder_weights"]


def swin_b(**kwargs) -> SwinTransformer:
    return _swin_b(**{"in_chans": 1, **kwargs})
