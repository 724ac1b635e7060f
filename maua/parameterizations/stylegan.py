"""maua/parameterizations/stylegan.py (an empty file in the reference): the StyleGAN2 latent parameterisation of maua_amd."""
from maua_amd.parameterizations import StyleGANParameterization  # noqa: F401
from maua_amd.projection import Projection, load, project  # noqa: F401
