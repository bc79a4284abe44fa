from ._mlpg import (MLPG, MLPGBatch, MultiStreamMLPG, UnitVarianceMLPG, UnitVarianceMLPGMSELoss, mlpg, mlpg_batch,  # noqa: F401
                    multi_stream_mlpg, unit_variance_mlpg, unit_variance_mlpg_mse_loss)
from ._modspec import ModSpec, ModSpecBatch, ModSpecMSELoss, modspec, modspec_batch, modspec_mse_loss  # noqa: F401
from ._trajectory import TrajectoryNLL, trajectory_nll  # noqa: F401
