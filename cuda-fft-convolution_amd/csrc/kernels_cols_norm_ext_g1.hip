// kernels_cols_norm_ext_g1.hip -- output-column kernels with the fused scale of normalised maps and the per-map extrema found in the store (fftconv_plan_set_extrema), fp32 maps,
// configurations of group 1 of fast_paths.hpp (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 1
#define FC_TU_NORM 1
#define FC_TU_EXTREMA 1
#include "kernels_cols_rect.inc"
