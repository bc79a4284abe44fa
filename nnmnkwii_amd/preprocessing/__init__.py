from .generic import (column_stats, delta_features, inv_minmax_scale, inv_scale, meanstd, meanvar, minmax, minmax_scale,  # noqa: F401
                      minmax_scale_params, scale, trim_zeros_frames)
from . import alignment  # noqa: F401
from .f0 import interp1d, interp1d_batch  # noqa: F401
from .modspec import inv_modspec, modphase, modspec, modspec_smoothing, modspec_smoothing_batch  # noqa: F401
