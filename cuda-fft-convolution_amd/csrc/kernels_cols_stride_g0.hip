// kernels_cols_stride_g0.hip -- output-column kernels with the strided store (fftconv_plan_set_output_stride), fp32 maps,
// configurations of group 0 of fast_paths.hpp (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 0
#define FC_TU_STRIDE 1
#include "kernels_cols_rect.inc"
