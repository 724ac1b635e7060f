"""Drop-in names for maua/GAN/metrics/: Frechet distance, kernel distance and precision / recall / density / coverage between the features
of real and of generated images, on the float64 matrix-core kernels of maua_amd.metrics."""
# compute and prdc are the submodules' names, as in the reference: from maua.GAN.metrics.compute import compute
from maua_amd.metrics import frechet_distance, kernel_distance  # noqa: F401
