// strip MLPG kernels compiled for the standard window set (strip_kernel<..., STD>): backward, double gradients in, float32 out (float64 out: the general kernel, see std_kernel)
#include "mlpg_strip_impl.h"
namespace mlpg {
namespace strip {
MLPG_STRIP_STD_KERNEL(double, float, true)
}  // namespace strip
}  // namespace mlpg
