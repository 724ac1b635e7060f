"""maua/GAN/decomposition/sefa.py's names on the device (apply_sefa's signature is adapted: see maua_amd.decomposition.apply_sefa)."""
from maua_amd.decomposition import apply_sefa, cff, sefa  # noqa: F401
