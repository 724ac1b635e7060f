"""``python -m maua.nca.generate STYLE OUT_DIR`` (maua/nca/generate.py's two positional arguments): the evolution, checkpoint-grid and
rate-map videos of OUT_DIR/<style name>_7500.pt."""
from maua_amd.nca import generate, generate_main, generate_parser, text_rate_map  # noqa: F401

if __name__ == "__main__":
    generate_main()
