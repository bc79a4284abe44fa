// strip MLPG kernels compiled for the standard window set (strip_kernel<..., STD>): forward, double
#include "mlpg_strip_impl.h"
namespace mlpg {
namespace strip {
MLPG_STRIP_STD_KERNEL(double, double, false)
}  // namespace strip
}  // namespace mlpg
