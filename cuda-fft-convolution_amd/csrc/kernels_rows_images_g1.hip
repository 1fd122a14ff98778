// kernels_rows_images_g1.hip -- image-walk spectral-row kernels, row lengths of group 1 of fast_paths.hpp
// (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 1
#include "kernels_rows_images.inc"
