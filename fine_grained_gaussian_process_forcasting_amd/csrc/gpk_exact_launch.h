// Exact forward: the per-unit launchers behind gpk_launch_exact (gpk_exact.hip). Each unit
// gpk_exact_nb*.hip instantiates gpk_exact_kernel (gpk_exact_kernel.h) for its own NB = ceil(N / 16)
// values and returns -6 for any other; the units are cut for similar compile times (~ NB^2 per kernel).
// NB = 16 shares its unit with NB = 9 on purpose (see gpk_exact_nb9_nb16.hip).
#pragma once
#include "gpk_internal.h"

int gpk_launch_exact_nb1_8(const GpkExactArgs& a, int NB, hipStream_t stream);
int gpk_launch_exact_nb10_11(const GpkExactArgs& a, int NB, hipStream_t stream);
int gpk_launch_exact_nb12_13(const GpkExactArgs& a, int NB, hipStream_t stream);
int gpk_launch_exact_nb14_15(const GpkExactArgs& a, int NB, hipStream_t stream);
int gpk_launch_exact_nb9_nb16(const GpkExactArgs& a, int NB, hipStream_t stream);   // + gpk_launch_exact_stamps
