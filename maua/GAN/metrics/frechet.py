"""maua/GAN/metrics/frechet.py's names on the device (symsqrtm raises NotImplementedError by name)."""
from maua_amd.metrics import frechet_distance, sqrtm, symsqrtm  # noqa: F401
