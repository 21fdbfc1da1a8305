// Which disparities belong to pixels the right camera cannot see (include/fsmi.h has the contract).
// One launch, three phases per block of whole rows:
//   stage     zero the rows' z-buffer in LDS, copy the right-view rows into LDS
//   splat     every in-view pixel atomicMax-es the bits of its disparity onto the z-buffer column it
//             lands on (a positive finite float's bits order like the float, so the maximum does not
//             depend on the order of arrival)
//   classify  one class per pixel, the optional error map, per-thread class counts
// and a count reduction: shuffle tree per wave, the four wave rows through LDS, one integer atomic per
// class per block.  Nothing in it depends on which block or lane runs first.
#include <climits>
#include <cstdint>
#include <type_traits>

#include "fsmi_common.h"

namespace fsmi {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxW = 8192;               // 8 B of LDS per column: a block stays at or below 64 KiB
constexpr int kBlockPixels = 1024;        // rows per block = clamp(kBlockPixels / W, 1, kMaxRows)
constexpr int kMaxRows = 8;
constexpr int kMaxBlocks = 2048;          // 256 CUs x 8 resident blocks; beyond it a block takes several row groups
constexpr int kNClass = FSMI_VIS_NCLASS;

struct Params {
  float occlusion_tol, lr_thresh;
  int H, W, rows_per_block, groups_per_pair, blocks_per_pair;
};

// f(i, integral_constant<int, K>): K = 4 for a quad of block-local pixels i .. i+3 whose global index
// is a multiple of 4 (16-byte aligned whatever the row base is), K = 1 for the at most 3 pixels in
// front of the first quad and the at most 3 behind the last.
template <class F>
__device__ __forceinline__ void sweep(int n, int head, F&& f) {
  const int nquad = (n - head) >> 2;
  for (int q = threadIdx.x; q < nquad; q += kThreads) f(head + 4 * q, std::integral_constant<int, 4>{});
  const int tail0 = head + 4 * nquad;
  const int nscalar = head + (n - tail0);                     // <= 6
  if (static_cast<int>(threadIdx.x) < nscalar) {
    const int t = threadIdx.x;
    f(t < head ? t : tail0 + (t - head), std::integral_constant<int, 1>{});
  }
}

template <int K>
__device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[K]) {
  if constexpr (K == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

// in view: finite, positive, and not left of the right image.  xr is fsmi.h's float(u) - d.
__device__ __forceinline__ int precheck(float d, int u, float& xr) {
#pragma clang fp contract(off)
  if (!(isfinite(d) && d > 0.f)) return FSMI_VIS_INVALID;
  xr = static_cast<float>(u) - d;
  return xr < 0.f ? FSMI_VIS_OUT_OF_VIEW : FSMI_VIS_VISIBLE;
}

// One group of whole rows: n pixels from flat index p0 of the maps.  Adds the group's classes to cnt.
template <bool OCC, bool RIGHT>
__device__ __forceinline__ void classify_group(const float* __restrict__ disp, const float* __restrict__ disp_right,
                                               unsigned char* __restrict__ classes, float* __restrict__ err,
                                               unsigned int* lds, int n, long long p0, const Params& p,
                                               int (&cnt)[kNClass]) {
  const int W = p.W;
  const int head = min(n, static_cast<int>((4 - (p0 & 3)) & 3));
  unsigned int* zbuf = lds;                                       // [n], OCC only
  float* right = reinterpret_cast<float*>(lds + (OCC ? n : 0));   // [n], RIGHT only
  disp += p0;

  if constexpr (OCC || RIGHT) {
    sweep(n, head, [&](int i, auto k) {
      constexpr int K = decltype(k)::value;
      if constexpr (OCC) {
#pragma unroll
        for (int j = 0; j < K; ++j) zbuf[i + j] = 0u;
      }
      if constexpr (RIGHT) {
        float v[K];
        load<K>(disp_right + p0 + i, v);
#pragma unroll
        for (int j = 0; j < K; ++j) right[i + j] = v[j];
      }
    });
    __syncthreads();
  }
  if constexpr (OCC) {
    sweep(n, head, [&](int i, auto k) {
      constexpr int K = decltype(k)::value;
      float d[K];
      load<K>(disp + i, d);
      int row = i / W, u = i - row * W;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        float xr;
        if (precheck(d[j], u, xr) == FSMI_VIS_VISIBLE) {
          // 0 <= xr <= u <= W - 1 and xr + 0.5f is exact or rounds down to 0.5f: c is in [0, W - 1]
          const int c = static_cast<int>(floorf(xr + 0.5f));
          atomicMax(&zbuf[row * W + c], __float_as_uint(d[j]));
        }
        if (++u == W) { u = 0; ++row; }
      }
    });
    __syncthreads();
  }

  sweep(n, head, [&](int i, auto k) {
#pragma clang fp contract(off)
    constexpr int K = decltype(k)::value;
    float d[K], e[K];
    unsigned char cls[K];
    load<K>(disp + i, d);
    int row = i / W, u = i - row * W;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      float xr;
      int c = precheck(d[j], u, xr);
      e[j] = __builtin_nanf("");
      if (c == FSMI_VIS_VISIBLE) {
        bool occluded = false, mismatch = false;
        if constexpr (OCC) {
          const int col = static_cast<int>(floorf(xr + 0.5f));
          occluded = __uint_as_float(zbuf[row * W + col]) - d[j] > p.occlusion_tol;
        }
        if constexpr (RIGHT) {
          const float* rr = right + row * W;
          const int x0 = static_cast<int>(floorf(xr));        // in [0, W - 1], as c above
          const float t = xr - static_cast<float>(x0);
          const int x1 = min(x0 + 1, W - 1);
          const float a = rr[x0];
          const float r = t == 0.f ? a : a + t * (rr[x1] - a);
          e[j] = fabsf(d[j] - r);
          mismatch = !(e[j] <= p.lr_thresh);
        }
        c = occluded ? FSMI_VIS_OCCLUDED : mismatch ? FSMI_VIS_MISMATCH : FSMI_VIS_VISIBLE;
      }
      cls[j] = static_cast<unsigned char>(c);
#pragma unroll
      for (int m = 0; m < kNClass; ++m) cnt[m] += c == m;
      if (++u == W) { u = 0; ++row; }
    }
    if constexpr (K == 4) {
      *reinterpret_cast<uchar4*>(classes + p0 + i) = make_uchar4(cls[0], cls[1], cls[2], cls[3]);
      if (err) *reinterpret_cast<float4*>(err + p0 + i) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
      classes[p0 + i] = cls[0];
      if (err) err[p0 + i] = e[0];
    }
  });
  __syncthreads();                                            // the z-buffer and the right rows are done with
}

// A block takes the row groups g, g + blocks_per_pair, ... of one pair and keeps its class counts in
// registers across them: the count atomics are per block, not per group.
template <bool OCC, bool RIGHT>
__global__ __launch_bounds__(kThreads) void visibility_kernel(const float* __restrict__ disp,
                                                              const float* __restrict__ disp_right,
                                                              unsigned char* __restrict__ classes,
                                                              float* __restrict__ err,
                                                              unsigned long long* __restrict__ counts, Params p) {
  extern __shared__ unsigned int lds[];
  const int b = blockIdx.x / p.blocks_per_pair;
  int cnt[kNClass] = {};
  for (int g = blockIdx.x - b * p.blocks_per_pair; g < p.groups_per_pair; g += p.blocks_per_pair) {
    const int r0 = g * p.rows_per_block;
    const int n = min(p.rows_per_block, p.H - r0) * p.W;      // <= 8192
    classify_group<OCC, RIGHT>(disp, disp_right, classes, err, lds, n, (static_cast<long long>(b) * p.H + r0) * p.W, p,
                               cnt);
  }

#pragma unroll
  for (int m = 0; m < kNClass; ++m)
    for (int off = kWave / 2; off > 0; off >>= 1) cnt[m] += __shfl_xor(cnt[m], off, kWave);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < kNClass; ++m) lds[wave * kNClass + m] = cnt[m];
  }
  __syncthreads();
  if (threadIdx.x < kNClass) {
    unsigned int s = 0;
    for (int w = 0; w < kThreads / kWave; ++w) s += lds[w * kNClass + threadIdx.x];
    if (s) atomicAdd(&counts[static_cast<long long>(b) * kNClass + threadIdx.x], static_cast<unsigned long long>(s));
  }
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" int fsmi_disp_visibility(const float* disp, const float* disp_right_or_null, unsigned char* classes,
                                    float* err_or_null, long long* counts, int B, int H, int W, float occlusion_tol,
                                    float lr_thresh, int occlusion, void* stream) {
  FSMI_CHECK_ARG(B > 0 && H > 0 && W > 0, "fsmi_disp_visibility: bad shape (%d,%d,%d)", B, H, W);
  FSMI_CHECK_ARG(W <= kMaxW, "fsmi_disp_visibility: W = %d exceeds %d (a row's z-buffer and right-view row live in LDS)",
                 W, kMaxW);
  FSMI_CHECK_ARG(disp && classes && counts, "fsmi_disp_visibility: null pointer");
  FSMI_CHECK_ARG(!err_or_null || disp_right_or_null, "fsmi_disp_visibility: the error map needs disp_right");
  FSMI_CHECK_ARG(!(occlusion_tol != occlusion_tol) && !(lr_thresh != lr_thresh),
                 "fsmi_disp_visibility: occlusion_tol, lr_thresh must not be NaN");
  FSMI_CHECK_ARG(aligned(disp, 16) && aligned(disp_right_or_null, 16) && aligned(err_or_null, 16) &&
                     aligned(classes, 4) && aligned(counts, 8),
                 "fsmi_disp_visibility: disp, disp_right, err must be 16-byte aligned, classes 4-byte, counts 8-byte");
  Params p;
  p.occlusion_tol = occlusion_tol;
  p.lr_thresh = lr_thresh;
  p.H = H;
  p.W = W;
  p.rows_per_block = std::min(std::max(kBlockPixels / W, 1), kMaxRows);
  p.groups_per_pair = (H + p.rows_per_block - 1) / p.rows_per_block;
  p.blocks_per_pair = std::min(p.groups_per_pair, std::max(kMaxBlocks / B, 1));
  const long long nblocks = static_cast<long long>(B) * p.blocks_per_pair;      // <= max(B, kMaxBlocks)
  const bool occ = occlusion != 0, right = disp_right_or_null != nullptr;
  // the count rows of the reduction reuse the front of the same array
  const size_t lds_bytes = std::max<size_t>(static_cast<size_t>(p.rows_per_block) * W * 4 * (int(occ) + int(right)),
                                            (kThreads / kWave) * kNClass * sizeof(unsigned int));
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemsetAsync(counts, 0, static_cast<size_t>(B) * kNClass * sizeof(long long), s);
  if (e != hipSuccess) {
    set_error("fsmi_disp_visibility: hipMemsetAsync failed: %s", hipGetErrorString(e));
    return static_cast<int>(e);
  }
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const dim3 grid(static_cast<unsigned>(nblocks)), block(kThreads);
#define FSMI_VIS_LAUNCH(OCC, RIGHT)                                                                          \
  hipLaunchKernelGGL((visibility_kernel<OCC, RIGHT>), grid, block, lds_bytes, s, disp, disp_right_or_null, \
                     classes, err_or_null, cnt, p)
  if (occ && right) FSMI_VIS_LAUNCH(true, true);
  else if (occ) FSMI_VIS_LAUNCH(true, false);
  else if (right) FSMI_VIS_LAUNCH(false, true);
  else FSMI_VIS_LAUNCH(false, false);
#undef FSMI_VIS_LAUNCH
  return finish_launch("fsmi_disp_visibility");
}
