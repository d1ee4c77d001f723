// Exact forward, NB = 14..15 (N = 209..240): this unit's instantiations of gpk_exact_kernel.
#include "gpk_exact_kernel.h"
#include "gpk_exact_launch.h"

int gpk_launch_exact_nb14_15(const GpkExactArgs& a, int NB, hipStream_t stream) {
  switch (NB) {
    case 14: return launch_exact_case<14>(a, stream);
    case 15: return launch_exact_case<15>(a, stream);
    default: return -6;
  }
}
