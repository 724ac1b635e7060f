"""Drop-in name for maua/diffusion/video.py: the optical-flow video pipeline around guided diffusion (:38-379: frames, the flow and
consistency cache, ``VideoFlowDiffusionProcessor``, ``video_sample``) with its command line, ``python -m maua.diffusion.video``.  The
latent / stable / glide / glid3xl processors and the neural flow models are not built and raise by name."""
from maua_amd.diffusion import get_diffusion_model  # noqa: F401
from maua_amd.flow import decode_mflo, encode_mflo, flow_warp_map, get_consistency_map, get_flow_model, warp  # noqa: F401
from maua_amd.video_diffusion import (FramesOnDisk, VideoFlowDiffusionProcessor, VideoFrames, WriteThread, build_parser,  # noqa: F401
                                      initialize_cache_files, initialize_optical_flow, main, seed_everything, video_sample)

if __name__ == "__main__":
    main()
