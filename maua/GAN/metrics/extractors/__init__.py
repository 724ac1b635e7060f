"""Drop-in names for maua/GAN/metrics/extractors/: ``get_extractor`` of maua_amd.metrics.  The SwAV ResNet-50 is built
(``"SwAV:<checkpoint>"``, weights from a local file: they are not bundled); the Inception extractor is not."""
from maua_amd.metrics import get_extractor  # noqa: F401
