// Exact forward, NB = 12..13 (N = 177..208): this unit's instantiations of gpk_exact_kernel.
#include "gpk_exact_kernel.h"
#include "gpk_exact_launch.h"

int gpk_launch_exact_nb12_13(const GpkExactArgs& a, int NB, hipStream_t stream) {
  switch (NB) {
    case 12: return launch_exact_case<12>(a, stream);
    case 13: return launch_exact_case<13>(a, stream);
    default: return -6;
  }
}
