"""``python -m maua.nca.train STYLE OUT_DIR`` (maua/nca/train.py's two positional arguments)."""
from maua_amd.nca import CA, load_ca, perception, save, to_rgb, train, train_main, train_parser  # noqa: F401

if __name__ == "__main__":
    train_main()
