from ._mlpg import (MLPG, MLPGBatch, UnitVarianceMLPG, UnitVarianceMLPGMSELoss, mlpg, mlpg_batch,  # noqa: F401
                    unit_variance_mlpg, unit_variance_mlpg_mse_loss)
from ._modspec import ModSpec, modspec  # noqa: F401
