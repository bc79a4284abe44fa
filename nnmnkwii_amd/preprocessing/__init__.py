from .generic import (column_stats, delta_features, inv_minmax_scale, inv_scale, meanstd, meanvar, minmax, minmax_scale,  # noqa: F401
                      minmax_scale_params, scale, trim_zeros_frames)
from . import alignment  # noqa: F401
from .f0 import interp1d, interp1d_batch  # noqa: F401
from .frames import joint_features_batch, remove_zeros_frames, remove_zeros_frames_batch  # noqa: F401
from .silence import remove_silence_frames, remove_silence_frames_batch  # noqa: F401
from .wave import (inv_mulaw, inv_mulaw_quantize, inv_preemphasis, mulaw, mulaw_quantize, preemphasis, wave_decode_batch,  # noqa: F401
                   wave_encode_batch)
from .modspec import inv_modspec, modphase, modspec, modspec_smoothing, modspec_smoothing_batch  # noqa: F401
