// Exact forward, NB = 10..11 (N = 145..176): this unit's instantiations of gpk_exact_kernel.
#include "gpk_exact_kernel.h"
#include "gpk_exact_launch.h"

int gpk_launch_exact_nb10_11(const GpkExactArgs& a, int NB, hipStream_t stream) {
  switch (NB) {
    case 10: return launch_exact_case<10>(a, stream);
    case 11: return launch_exact_case<11>(a, stream);
    default: return -6;
  }
}
