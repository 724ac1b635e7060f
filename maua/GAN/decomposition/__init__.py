"""maua/GAN/decomposition: latent directions on the device (maua_amd.decomposition)."""
from maua_amd.decomposition import Directions, apply_sefa, cff, eigh, ganspace, load, sefa, svd, svdvals  # noqa: F401
