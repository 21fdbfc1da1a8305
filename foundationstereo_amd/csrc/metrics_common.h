// Per-pixel rules shared by the scoring kernels (metrics.hip, seq_metrics.hip): the ground truth's
// decode and the validity of a pixel, as include/fsmi.h states them.
#pragma once

#include "fsmi_common.h"

namespace fsmi {

// depth_uint8_decoding (Utils.py:137-140): float32 of the reference's float64 result
__device__ __forceinline__ float decode_gt(unsigned r, unsigned g, unsigned b, double gt_scale) {
  const int n = static_cast<int>(r * 65025u + g * 255u + b);          // <= 16 605 816
  return static_cast<float>(static_cast<double>(n) / gt_scale);
}

// the mask alone decides when there is one; otherwise gt > 0 and finite
__device__ __forceinline__ bool pixel_valid(bool has_mask, unsigned char m, float gt) {
  return has_mask ? m != 0 : (gt > 0.f && gt < INFINITY);
}

}  // namespace fsmi
