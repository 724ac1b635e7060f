"""Drop-in name for maua/diffusion/image.py: get_diffusion_model for the guided processor (:77-129, the grad-module list around
GuidedDiffusion) and the multi-resolution image pipeline around it (:30-74, 132-323: init image, a schedule of sizes and skip
fractions, optional RealESRGAN up-scaling and lanczos3 resizing between scales, blended tiles for large images) with its command line,
``python -m maua.diffusion.image``.  The latent / stable / glide / glid3xl processors and the SwinIR up-scalers are not built and raise."""
from maua_amd.diffusion import get_diffusion_model  # noqa: F401
from maua_amd.image import (MultiResolutionDiffusionProcessor, build_output_name, get_start_steps, image_sample,  # noqa: F401
                            initialize_image, main, round64, width_height)

if __name__ == "__main__":
    main()
