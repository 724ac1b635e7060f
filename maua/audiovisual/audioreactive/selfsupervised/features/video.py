"""Drop-in name for maua/audiovisual/audioreactive/selfsupervised/features/video.py: re-exports the MI355X-native implementation in maua_amd."""
from maua_amd.video_features import (absdiff, adaptive_freq_rms, blueogram, directogram, fft, greenogram, high_freq_rms,  # noqa: F401
                                     hsv_hist, huestogram, low_freq_rms, mid_freq_rms, optical_flow_cpu, redogram, rgb_hist, saturogram,
                                     valueogram, video_flow_onsets, video_spectral_onsets, video_spectrogram, visual_variance)
