// How good is a disparity map: per-pair EPE, RMSE, bad-pixel rates and KITTI's D1 against a ground
// truth, plus the prediction's own statistics (train/utils.py:88-141 compute_stereo_metrics and
// train/losses.py:326-339 monitoring_stereo, which gather through a boolean mask, loop over the batch
// in Python and synchronise the host 4 + K times per pair).  Here: one streaming pass and a tiny
// second kernel, no host synchronisation, no allocation, capturable in a hipGraph.
//   disp_metrics_partial   grid (NB, B): a block reduces its pixels of pair b into one row of 17 doubles
//                          and STORES it (the fixed-order reduction of metrics_common.h; here the order
//                          of every addition is a function of (H*W, NB) alone)
//   disp_metrics_finalize  one block per pair: sums the NB rows in a fixed order, writes the raw
//                          accumulators and the table of metrics
//   gt_decode              the reference's 3 x uint8 ground-truth encoding (Utils.py:137-140) -> fp32
// Per-pixel arithmetic is un-contracted fp32, as torch evaluates |pred - gt| > t on fp32 tensors; every
// sum is fp64 ((double)e * (double)e is exact), counts are exact integers held as doubles.
#include <climits>
#include <cstdint>

#include "metrics_common.h"

namespace fsmi {
namespace {

constexpr int NACC = FSMI_METRICS_NACC;
constexpr int MAXT = FSMI_METRICS_MAX_THRESHOLDS;
constexpr int kQuadsPerBlock = 1024;      // 256 lanes x 4 quads of 4 pixels
constexpr int kMaxBlocks = 512;           // per pair; the finalize kernel reads at most 2 rows per lane

static_assert(NACC == 9 + MAXT, "accumulator layout: 9 fixed slots then the thresholds");

enum { A_N = 0, A_SE, A_SE2, A_D1, A_NONFINITE, A_SX, A_SX2, A_MIN, A_MAX, A_BAD };

struct Metrics {
  long long P;            // H * W
  double gt_scale;
  float thr[MAXT];        // unused slots +inf: e > +inf never counts
};

// min / max that propagate NaN (fminf / fmaxf return the other operand): once NaN, always NaN
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// the reduction's combine (metrics_common.h): the two extreme slots by comparison, every other one a sum
struct Combine {
  __device__ __forceinline__ double operator()(int slot, double a, double b) const {
    return slot == A_MIN ? nan_min(a, b) : slot == A_MAX ? nan_max(a, b) : a + b;
  }
};
constexpr Combine combine{};

// One lane's running row.  Counts stay below 2^32 per lane (a pair has at most 2^31 - 1 pixels).
struct Lane {
  double se = 0.0, se2 = 0.0, sx = 0.0, sx2 = 0.0;
  unsigned n = 0, d1 = 0, nonfinite = 0, bad[MAXT] = {};
  float mn = INFINITY, mx = -INFINITY;
};

// returns the error-map value of the pixel: e where valid, +inf where not
__device__ __forceinline__ float take(Lane& a, float x, float gt, bool has_mask, unsigned char m, float x0,
                                      const Metrics& g) {
#pragma clang fp contract(off)
  const double dx = static_cast<double>(x) - static_cast<double>(x0);
  a.sx += dx;
  a.sx2 += dx * dx;
  a.mn = (x < a.mn || x != x) ? x : a.mn;
  a.mx = (x > a.mx || x != x) ? x : a.mx;
  const bool valid = pixel_valid(has_mask, m, gt);
  if (!valid) return INFINITY;
  const float e = fabsf(x - gt);
  const double ed = static_cast<double>(e);
  a.n += 1;
  a.se += ed;
  a.se2 += ed * ed;
  a.d1 += (e > 3.0f && e > __fmul_rn(0.05f, fabsf(gt))) ? 1u : 0u;
  a.nonfinite += !(e < INFINITY) ? 1u : 0u;                          // NaN or inf
#pragma unroll
  for (int k = 0; k < MAXT; ++k) a.bad[k] += e > g.thr[k] ? 1u : 0u;   // NaN > t is false: "not bad"
  return e;
}

// grid (NB, B); the blocks of one pair stride over its quads.  A pair starts at b * P pixels, which is
// 16-byte aligned in the fp32 maps (4-byte in the mask, 12-byte quads in the u8 ground truth) only
// when that is a multiple of 4: up to 3 head pixels and P' % 4 tail pixels are taken one by one by
// block 0, everything between them as 4-wide groups that never leave the pair.
template <bool U8GT>
__global__ __launch_bounds__(256) void disp_metrics_partial_kernel(const float* __restrict__ pred,
                                                                   const void* __restrict__ gt_any,
                                                                   const unsigned char* __restrict__ mask,
                                                                   double* __restrict__ partials,
                                                                   float* __restrict__ error, Metrics g) {
  __shared__ double lds[4][NACC];
  const int b = blockIdx.y;
  const long long P = g.P, start = b * P;
  const float* p = pred + start;
  const GroundTruth<U8GT> gt(gt_any, start, g.gt_scale);
  const unsigned char* mk = mask ? mask + start : nullptr;
  float* er = error ? error + start : nullptr;
  const bool has_mask = mask != nullptr;
  const float x0 = p[0];

  const long long head = min(P, static_cast<long long>((4 - (start & 3)) & 3));
  const long long nquad = (P - head) >> 2;
  const long long tail = head + (nquad << 2);
  const long long t = blockIdx.x * 256ll + threadIdx.x, stride = gridDim.x * 256ll;

  Lane a;
  auto one = [&](long long i) {                                      // pixel i of the pair, i < P
    const float gti = gt[i];
    const float e = take(a, p[i], gti, has_mask, has_mask ? mk[i] : 0, x0, g);
    if (er) er[i] = e;
  };
  if (t < head) one(t);
  for (long long q = t; q < nquad; q += stride) {
    const long long i = head + (q << 2);
    const float4 x = *reinterpret_cast<const float4*>(p + i);
    const float4 g4 = gt.quad(i);
    const unsigned m4 = has_mask ? *reinterpret_cast<const unsigned*>(mk + i) : 0u;
    float4 e;
    e.x = take(a, x.x, g4.x, has_mask, m4 & 255u, x0, g);
    e.y = take(a, x.y, g4.y, has_mask, (m4 >> 8) & 255u, x0, g);
    e.z = take(a, x.z, g4.z, has_mask, (m4 >> 16) & 255u, x0, g);
    e.w = take(a, x.w, g4.w, has_mask, m4 >> 24, x0, g);
    if (er) *reinterpret_cast<float4*>(er + i) = e;
  }
  if (tail + t < P) one(tail + t);

  double v[NACC];
  v[A_N] = a.n; v[A_SE] = a.se; v[A_SE2] = a.se2; v[A_D1] = a.d1; v[A_NONFINITE] = a.nonfinite;
  v[A_SX] = a.sx; v[A_SX2] = a.sx2; v[A_MIN] = a.mn; v[A_MAX] = a.mx;
#pragma unroll
  for (int k = 0; k < MAXT; ++k) v[A_BAD + k] = a.bad[k];
  const double r = block_reduce(v, lds, combine);
  if (threadIdx.x < NACC)
    partials[(static_cast<long long>(b) * gridDim.x + blockIdx.x) * NACC + threadIdx.x] = r;
}

// One block per pair.  Lane t sums rows t, t + 256, ... (in index order) of the pair's NB partial
// rows, then the same block_reduce.  Lane 0 turns the accumulators into the table.
__global__ __launch_bounds__(256) void disp_metrics_finalize_kernel(const double* __restrict__ partials,
                                                                    const float* __restrict__ pred,
                                                                    double* __restrict__ sums,
                                                                    double* __restrict__ table, int NB, long long P) {
#pragma clang fp contract(off)
  __shared__ double lds[4][NACC];
  __shared__ double row[NACC];
  const int b = blockIdx.x;
  double v[NACC];
#pragma unroll
  for (int s = 0; s < NACC; ++s) v[s] = s == A_MIN ? INFINITY : s == A_MAX ? -INFINITY : 0.0;
  for (int r = threadIdx.x; r < NB; r += 256) {
    const double* src = partials + (static_cast<long long>(b) * NB + r) * NACC;
#pragma unroll
    for (int s = 0; s < NACC; ++s) v[s] = combine(s, v[s], src[s]);
  }
  const double r = block_reduce(v, lds, combine);
  if (threadIdx.x < NACC) {
    sums[b * NACC + threadIdx.x] = r;
    row[threadIdx.x] = r;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* o = table + b * NACC;
  const double n = row[A_N], Pd = static_cast<double>(P);
  const bool any = n > 0.0;                                          // train/utils.py:122-123: an empty mask scores 0
  o[0] = n;
  o[1] = any ? row[A_SE] / n : 0.0;
  o[2] = any ? sqrt(row[A_SE2] / n) : 0.0;
  o[3] = any ? row[A_D1] / n : 0.0;
  o[4] = row[A_NONFINITE];
  const double x0 = static_cast<double>(pred[b * P]);
  o[5] = x0 + row[A_SX] / Pd;
  // unbiased.  A difference that rounds below 0 on a near-constant map is 0 (torch's two-pass value is
  // never negative); the comparison, unlike fmax, keeps NaN, and one pixel stays 0 / 0 = NaN
  const double dev2 = row[A_SX2] - row[A_SX] * row[A_SX] / Pd;
  o[6] = sqrt((dev2 < 0.0 ? 0.0 : dev2) / (Pd - 1.0));
  o[7] = row[A_MIN];
  o[8] = row[A_MAX];
  for (int k = 0; k < MAXT; ++k) o[9 + k] = any ? row[A_BAD + k] / n : 0.0;
}

// 4 pixels (12 bytes) per lane over the flat (B*H*W) index; the lane after the last quad takes the rest
__global__ __launch_bounds__(256) void gt_decode_kernel(const unsigned char* __restrict__ u8, float* __restrict__ out,
                                                        long long N, double gt_scale) {
  const long long q = blockIdx.x * 256ll + threadIdx.x;
  const long long nquad = N >> 2;
  if (q > nquad) return;
  const long long i = q << 2;
  if (q < nquad) {
    *reinterpret_cast<float4*>(out + i) = decode_gt4(u8 + 3 * i, gt_scale);
  } else {
    for (long long k = i; k < N; ++k) out[k] = decode_gt(u8[3 * k], u8[3 * k + 1], u8[3 * k + 2], gt_scale);
  }
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" {

int fsmi_disp_metrics_blocks(int H, int W) {
  if (H < 1 || W < 1) return 1;
  const long long quads = (static_cast<long long>(H) * W + 3) >> 2;
  return static_cast<int>(std::min<long long>(std::max<long long>((quads + kQuadsPerBlock - 1) / kQuadsPerBlock, 1),
                                              kMaxBlocks));
}

int fsmi_disp_metrics(const float* pred, const float* gt, const unsigned char* gt_u8, const unsigned char* mask,
                      const float* thresholds, int K, double gt_scale, double* partials, double* sums, double* table,
                      float* error, int B, int H, int W, void* stream) {
  Metrics g;
  if (const int e = check_scoring_args("fsmi_disp_metrics", B, H, W, gt, gt_u8, gt_scale, thresholds, K, g.thr)) return e;
  FSMI_CHECK_ARG(pred && partials && sums && table, "fsmi_disp_metrics: null pointer");
  FSMI_CHECK_ARG(aligned(pred, 16) && (!gt || aligned(gt, 16)) && (!gt_u8 || aligned(gt_u8, 4)) &&
                     (!mask || aligned(mask, 4)) && (!error || aligned(error, 16)) && aligned(partials, 8) &&
                     aligned(sums, 8) && aligned(table, 8),
                 "fsmi_disp_metrics: fp32 maps must be 16-byte, uint8 maps 4-byte, fp64 outputs 8-byte aligned");
  g.P = static_cast<long long>(H) * W;
  g.gt_scale = gt_scale;
  const int NB = fsmi_disp_metrics_blocks(H, W);
  hipStream_t s = as_stream(stream);
  if (gt_u8)
    hipLaunchKernelGGL(disp_metrics_partial_kernel<true>, dim3(NB, B), dim3(256), 0, s, pred,
                       static_cast<const void*>(gt_u8), mask, partials, error, g);
  else
    hipLaunchKernelGGL(disp_metrics_partial_kernel<false>, dim3(NB, B), dim3(256), 0, s, pred,
                       static_cast<const void*>(gt), mask, partials, error, g);
  hipLaunchKernelGGL(disp_metrics_finalize_kernel, dim3(B), dim3(256), 0, s, partials, pred, sums, table, NB, g.P);
  return finish_launch("fsmi_disp_metrics");
}

int fsmi_gt_decode(const unsigned char* gt_u8, float* out, int B, int H, int W, double gt_scale, void* stream) {
  FSMI_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "fsmi_gt_decode: bad shape (%d,%d,%d)", B, H, W);
  FSMI_CHECK_ARG(gt_scale > 0.0, "fsmi_gt_decode: gt_scale = %g must be positive", gt_scale);
  FSMI_CHECK_ARG(gt_u8 && out, "fsmi_gt_decode: null pointer");
  const long long N = static_cast<long long>(B) * H * W;
  FSMI_CHECK_ARG(((N >> 2) + 256) / 256 <= INT_MAX, "fsmi_gt_decode: too many pixels");
  FSMI_CHECK_ARG(aligned(gt_u8, 4) && aligned(out, 16), "fsmi_gt_decode: gt_u8 must be 4-byte and out 16-byte aligned");
  hipLaunchKernelGGL(gt_decode_kernel, dim3(ceil_div((N >> 2) + 1, 256)), dim3(256), 0, as_stream(stream), gt_u8, out, N,
                     gt_scale);
  return finish_launch("fsmi_gt_decode");
}

}  // extern "C"
