"""Drop-in names for maua/nca/ (after znah's gitart_kunstformen_ca): the cellular automaton's rule, its checkpoints and the three videos
of generate.py and the training loop of train.py, on the device kernels of maua_amd.nca."""
from maua_amd.nca import CA, generate, load_ca, perception, save, to_rgb, train  # noqa: F401
