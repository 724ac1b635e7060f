"""maua/GAN/metrics/prdc.py's names on the device."""
from maua_amd.metrics import nearest_neighbor_distances, pairwise_distances, prdc  # noqa: F401
