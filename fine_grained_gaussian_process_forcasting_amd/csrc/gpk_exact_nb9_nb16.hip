// Exact forward, NB = 16 (N = 241..256) and NB = 9 (N = 129..144): this unit's instantiations of
// gpk_exact_kernel. NB = 9 rides along so that the callers of the NB-taking helpers
// (exact_lds_layout, frag_index, hfrag_index) disagree on NB as they did in the single file: alone
// in a unit, the NB = 16 kernels are specialised on it and come out with other register counts
// (DESIGN.md section 8 item 8). With NB = 9 all nine kernels here are the single file's, byte for byte.
#include "gpk_exact_kernel.h"
#include "gpk_exact_launch.h"

int gpk_launch_exact_nb9_nb16(const GpkExactArgs& a, int NB, hipStream_t stream) {
  switch (NB) {
    case 9: return launch_exact_case<9>(a, stream);
    case 16: return launch_exact_case<16>(a, stream);
    default: return -6;
  }
}

// The stamps instantiation (gpk_debug_exact_stamps, scripts/stamps_exact.py): N = 256 only.
int gpk_launch_exact_stamps(const GpkExactArgs& a, unsigned long long* stamps, hipStream_t stream) {
  if (a.N != 256) return -6;
  return launch_exact_nb<16, true, true>(a, stamps, stream);
}
