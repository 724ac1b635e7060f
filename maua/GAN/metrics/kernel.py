"""maua/GAN/metrics/kernel.py's name on the device."""
from maua_amd.metrics import kernel_distance  # noqa: F401
