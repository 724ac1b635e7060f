"""Drop-in name for maua/GAN/generate_images.py: `python -m maua.GAN.generate_images --model_file ... --latent_sampling langevin
--langevin_critic "<text>"` (StyleGAN2 generators; maua_amd.sampling)."""
from maua_amd.sampling import build_parser, generate_images, main  # noqa: F401

if __name__ == "__main__":
    main()
