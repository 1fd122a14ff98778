// kernels_cols_rect16_g1.hip -- output-column kernels with the rectangle store (fftconv_plan_set_output_rect), 16-bit maps
// (plan option "map_format"), configurations of group 1 of fast_paths.hpp.
#define FC_TU_GROUP 1
#define FC_TU_OUT16 1
#include "kernels_cols_rect.inc"
