// kernels_cols16_g0.hip -- output-column kernels with 16-bit maps (plan option "map_format"), configurations of group 0 of
// fast_paths.hpp (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 0
#define FC_TU_OUT16 1
#include "kernels_cols.inc"
