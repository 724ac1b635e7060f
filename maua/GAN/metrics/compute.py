"""``python -m maua.GAN.metrics.compute --data_dir DIR --checkpoint CKPT`` (maua/GAN/metrics/compute.py's flags, --extractor widened to
CLIP:<tower> / SwAV:<checkpoint> and --allow_random_init added): the metrics of a generator checkpoint against a folder of real images, as JSON."""
from maua_amd.metrics import (EXTENSIONS, SIZE, FolderImages, GeneratorImages, compute, get_extractor, main, parser,  # noqa: F401
                              resize_clean, resize_single_channel)

if __name__ == "__main__":
    main()
