// kernels_rows_g2.hip -- one-map spectral-row and forward image-row kernels, configurations of group 2 of fast_paths.hpp
// (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 2
#include "kernels_rows.inc"
