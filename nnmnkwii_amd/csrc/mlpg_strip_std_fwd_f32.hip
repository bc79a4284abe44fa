// strip MLPG kernels compiled for the standard window set (strip_kernel<..., STD>): forward, float
#include "mlpg_strip_impl.h"
namespace mlpg {
namespace strip {
MLPG_STRIP_STD_KERNEL(float, float, false)
}  // namespace strip
}  // namespace mlpg
