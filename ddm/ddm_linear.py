"""Dotted-path alias so YAML `class_name: ddm.ddm_linear.DDPM` resolves to the HIP implementation."""
from adm_amd.ddm.ddm_linear import DDPM  # noqa: F401
