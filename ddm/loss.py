"""Dotted-path alias so the reference's `ddm.loss.LPIPSWithDiscriminator` resolves to the HIP implementation."""
from adm_amd.ddm.loss import LPIPSWithDiscriminator, NLayerDiscriminator, adopt_weight, weights_init  # noqa: F401
