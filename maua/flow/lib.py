"""Drop-in name for maua/flow/lib.py:18-80: the ``.mflo`` flow encoding, ``flow_warp_map`` and ``get_consistency_map``."""
from maua_amd.flow import check_consistency, decode_mflo, encode_mflo, flow_warp_map, get_consistency_map  # noqa: F401
