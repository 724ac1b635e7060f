"""Drop-in names for maua/GAN/metrics/extractors/swav.py: ``SwAV(checkpoint)`` is the reference's ``SwAV()`` with the weights read from
a local file (nothing is downloaded), ``ResNetFeatures`` its ResNet(Bottleneck, layers) backbone on the library's HIP kernels."""
from maua_amd.resnet import ResNetFeatures, SwAV  # noqa: F401
