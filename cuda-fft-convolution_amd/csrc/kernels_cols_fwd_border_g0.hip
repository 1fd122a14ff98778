// kernels_cols_fwd_border_g0.hip -- forward-column kernels of an image with a border (fftconv_plan_set_border), configurations of group 0 of fast_paths.hpp
// (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 0
#include "kernels_cols_fwd_border.inc"
