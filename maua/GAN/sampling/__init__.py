"""Drop-in names for maua/GAN/sampling/: Langevin sampling of latents against a critic, jacobian-norm rejection, sample_latents - on the
hand-written generator gradient of maua_amd (maua_amd.sampling)."""
from maua_amd.sampling import jacobian_norm_rejection, langevin_with_critic, sample_latents  # noqa: F401
