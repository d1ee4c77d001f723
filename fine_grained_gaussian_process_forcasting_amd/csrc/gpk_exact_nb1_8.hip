// Exact forward, NB = 1..8 (N = 1..128): this unit's instantiations of gpk_exact_kernel.
#include "gpk_exact_kernel.h"
#include "gpk_exact_launch.h"

int gpk_launch_exact_nb1_8(const GpkExactArgs& a, int NB, hipStream_t stream) {
  switch (NB) {
    case 1: return launch_exact_case<1>(a, stream);
    case 2: return launch_exact_case<2>(a, stream);
    case 3: return launch_exact_case<3>(a, stream);
    case 4: return launch_exact_case<4>(a, stream);
    case 5: return launch_exact_case<5>(a, stream);
    case 6: return launch_exact_case<6>(a, stream);
    case 7: return launch_exact_case<7>(a, stream);
    case 8: return launch_exact_case<8>(a, stream);
    default: return -6;
  }
}
