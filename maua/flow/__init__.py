"""Drop-in name for what the video pipeline uses of maua/flow/__init__.py: ``get_flow_model`` (:9-64) for its default list,
["farneback"] - estimated on the device, restated from the published algorithm - and the consistency / warp-map helpers it re-exports
(:67-68).  The neural flow models, ``preprocess_optical_flow`` and flow/utils.py are not built."""
from maua_amd.flow import check_consistency, flow_warp_map, get_consistency_map, get_flow_model  # noqa: F401
