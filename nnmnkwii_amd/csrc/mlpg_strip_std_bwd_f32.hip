// strip MLPG kernels compiled for the standard window set (strip_kernel<..., STD>): backward, float gradients in, float32 or float64 out
#include "mlpg_strip_impl.h"
namespace mlpg {
namespace strip {
MLPG_STRIP_STD_KERNEL(float, float, true)
MLPG_STRIP_STD_KERNEL(float, double, true)
}  // namespace strip
}  // namespace mlpg
