// Rules shared by the scoring kernels (metrics.hip, seq_metrics.hip, photometric.hip): the fixed-order
// fp64 reduction, the ground truth's decode and the validity of a pixel, as include/fsmi.h states them,
// and the check of the arguments the two ground-truth entry points have in common.
#pragma once

#include <climits>

#include "fsmi_common.h"

namespace fsmi {

// ---- the reduction.  Every sum of the scoring kernels is fp64 and STORED, never added atomically, and
// the order of its additions is a function of the lane index alone: a __shfl_down tree inside each wave
// (offsets 32, 16, .. 1), then the block's four waves through LDS as ((w0 + w1) + w2) + w3.  The same
// input therefore gives the same bits on any device.  Combine is (slot, a, b) -> double, a + b by
// default; whatever it is, it is applied in that same order.
struct SlotSum {
  __device__ __forceinline__ double operator()(int, double a, double b) const { return a + b; }
};

// the wave's 64 rows of N values -> lane 0's
template <int N, class Combine = SlotSum>
__device__ __forceinline__ void wave_reduce(double (&v)[N], Combine op = Combine()) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[s] = op(s, v[s], __shfl_down(v[s], off, 64));
  }
}

// the 256 lanes' rows of N values -> one row: lane s < N returns slot s (the others 0)
template <int N, int LD, class Combine = SlotSum>
__device__ __forceinline__ double block_reduce(double (&v)[N], double (*lds)[LD], Combine op = Combine()) {
  static_assert(N <= LD, "an LDS row holds every slot");
  wave_reduce(v, op);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int s = 0; s < N; ++s) lds[threadIdx.x >> 6][s] = v[s];
  }
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < N) {
    const int s = threadIdx.x;
    r = op(s, op(s, op(s, lds[0][s], lds[1][s]), lds[2][s]), lds[3][s]);
  }
  return r;
}

// ---- pixels

// four interleaved 3-byte pixels in three words, r g b r | g b r g | b r g b -> c[pixel][channel]
__device__ __forceinline__ void unpack_rgb4(const uint3& w, unsigned (&c)[4][3]) {
  c[0][0] = w.x & 255u; c[0][1] = (w.x >> 8) & 255u; c[0][2] = (w.x >> 16) & 255u;
  c[1][0] = w.x >> 24; c[1][1] = w.y & 255u; c[1][2] = (w.y >> 8) & 255u;
  c[2][0] = (w.y >> 16) & 255u; c[2][1] = w.y >> 24; c[2][2] = w.z & 255u;
  c[3][0] = (w.z >> 8) & 255u; c[3][1] = (w.z >> 16) & 255u; c[3][2] = w.z >> 24;
}

// depth_uint8_decoding (Utils.py:137-140): float32 of the reference's float64 result
__device__ __forceinline__ float decode_gt(unsigned r, unsigned g, unsigned b, double gt_scale) {
  const int n = static_cast<int>(r * 65025u + g * 255u + b);          // <= 16 605 816
  return static_cast<float>(static_cast<double>(n) / gt_scale);
}

// four encoded pixels from a 4-byte aligned address
__device__ __forceinline__ float4 decode_gt4(const unsigned char* p, double gt_scale) {
  unsigned c[4][3];
  unpack_rgb4(*reinterpret_cast<const uint3*>(p), c);
  return make_float4(decode_gt(c[0][0], c[0][1], c[0][2], gt_scale), decode_gt(c[1][0], c[1][1], c[1][2], gt_scale),
                     decode_gt(c[2][0], c[2][1], c[2][2], gt_scale), decode_gt(c[3][0], c[3][1], c[3][2], gt_scale));
}

// One pair's ground truth in either encoding, fp32 (H,W) or uint8 (H,W,3): gt is the batch's base,
// start the pair's first pixel.
template <bool U8>
struct GroundTruth {
  const float* f;
  const unsigned char* u;
  double scale;
  __device__ __forceinline__ GroundTruth(const void* gt, long long start, double gt_scale)
      : f(U8 ? nullptr : static_cast<const float*>(gt) + start),
        u(U8 ? static_cast<const unsigned char*>(gt) + 3 * start : nullptr), scale(gt_scale) {}
  __device__ __forceinline__ float operator[](long long i) const {
    return U8 ? decode_gt(u[3 * i], u[3 * i + 1], u[3 * i + 2], scale) : f[i];
  }
  // pixels i .. i + 3, where &f[i] is 16-byte (&u[3 * i] 4-byte) aligned
  __device__ __forceinline__ float4 quad(long long i) const {
    return U8 ? decode_gt4(u + 3 * i, scale) : *reinterpret_cast<const float4*>(f + i);
  }
};

// the mask alone decides when there is one; otherwise gt > 0 and finite
__device__ __forceinline__ bool pixel_valid(bool has_mask, unsigned char m, float gt) {
  return has_mask ? m != 0 : (gt > 0.f && gt < INFINITY);
}

// ---- host: what fsmi_disp_metrics and fsmi_seq_metrics (`who`) ask of the arguments they share.
// Fills thr with the K thresholds and +inf in the unused slots (e > +inf never counts).  FSMI_OK, or
// FSMI_ERR_ARG with the message set.
inline int check_scoring_args(const char* who, int B, int H, int W, const float* gt, const unsigned char* gt_u8,
                              double gt_scale, const float* thresholds, int K,
                              float (&thr)[FSMI_METRICS_MAX_THRESHOLDS]) {
  constexpr int MAXT = FSMI_METRICS_MAX_THRESHOLDS;
  FSMI_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "%s: bad shape (%d,%d,%d)", who, B, H, W);
  FSMI_CHECK_ARG(K >= 0 && K <= MAXT, "%s: K = %d thresholds: 0..%d", who, K, MAXT);
  FSMI_CHECK_ARG(K == 0 || thresholds, "%s: null thresholds with K = %d", who, K);
  FSMI_CHECK_ARG((gt != nullptr) != (gt_u8 != nullptr), "%s: exactly one of gt (fp32) and gt_u8", who);
  FSMI_CHECK_ARG(!gt_u8 || gt_scale > 0.0, "%s: gt_scale = %g must be positive", who, gt_scale);
  const long long P = static_cast<long long>(H) * W;
  FSMI_CHECK_ARG(P <= INT_MAX, "%s: H*W = %lld exceeds 2^31 - 1", who, P);
  for (int k = 0; k < MAXT; ++k) thr[k] = k < K ? thresholds[k] : INFINITY;
  return FSMI_OK;
}

}  // namespace fsmi
