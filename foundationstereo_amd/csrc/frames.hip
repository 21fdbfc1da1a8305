// The two ends of the demo around the forward.  Before it: two uint8 camera frames -> the fp32
// (B,2,3,Hp,Wp) batch the model consumes (scripts/run_demo.py:131-159: gray / RGBA handling,
// cv2.resize by --scale, uint8 HWC -> float CHW, InputPadder's replicate padding).  After it: the
// disparity picture (vis_disparity, Utils.py:108-133, called at run_demo.py:168-170).  Three kernels,
// all memory-bound streams:
//   frames_ingest   each source byte read once at scale 1 (4 taps per pixel otherwise) + 12 B written
//                   per padded pixel, as three float4 stores per lane
//   disp_minmax     4 B read per pixel; wave + block reduction, two integer atomics per block
//   disp_colorize   4 B read + 3 B written per pixel (+ 3 B read and written for the side-by-side image)
// Two definitions where the reference's behaviour is undefined: a NaN disparity is an invalid pixel
// (the reference's min() would return NaN and its uint8 cast is undefined), and max == min maps every
// valid pixel to LUT entry 0 (the reference divides by zero).
#include <climits>
#include <cstdint>

#include "fsmi_common.h"

namespace fsmi {
namespace {

struct Ingest {
  int H, W, C;            // source frame
  int Hs, Ws;             // resized frame
  int Hp, Wp;             // padded frame
  int top, left;          // InputPadder's pads in front of the resized frame
  double scale;
};

// Channel c of the resized frame's pixel (ys, xs).  RESIZE = false: the source byte itself.
// RESIZE = true: cv2.INTER_LINEAR without antialiasing, half-pixel centres, both taps clamped; the
// tap position in fp64 (cv2 computes it in double), the blend in un-contracted fp32, half rounded up
// (cv2's (sum + half) >> shift).  The result is an integer, as in the reference, which resizes uint8.
struct RowTaps {
  const unsigned char *r0, *r1;   // the two source rows
  float wy;
};

__device__ __forceinline__ void taps(int o, int n, double scale, int& i0, int& i1, float& w) {
  const double s = (static_cast<double>(o) + 0.5) / scale - 0.5;
  const double f = floor(s);
  w = static_cast<float>(s - f);
  const int i = static_cast<int>(fmin(fmax(f, -1.0), static_cast<double>(n)));   // in int range for any scale
  i0 = min(max(i, 0), n - 1);
  i1 = min(max(i + 1, 0), n - 1);
}

__device__ __forceinline__ float blend(float a, float b, float c, float d, float wx, float wy) {
#pragma clang fp contract(off)
  const float top = a + (b - a) * wx;
  const float bot = c + (d - c) * wx;
  const float v = top + (bot - top) * wy;
  return fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
}

// One lane owns 4 consecutive columns of one padded row of one image (Wp % 4 == 0): three float4
// stores, one per channel plane.  Source rows are C * W bytes and not aligned in general, so the
// source is read with byte loads; every index is clamped into the frame.  Image 2b is the left
// frame of pair b and 2b + 1 the right one: out is (B,2,3,Hp,Wp).  u8 (optional) receives the
// resized, unpadded left frame as (B,Hs,Ws,3); each of its pixels is owned by exactly one lane.
template <bool RESIZE>
__global__ __launch_bounds__(256) void frames_ingest_kernel(const unsigned char* __restrict__ left,
                                                            const unsigned char* __restrict__ right,
                                                            float* __restrict__ out, unsigned char* __restrict__ u8,
                                                            long long nquad, Ingest g) {
  const long long q = blockIdx.x * 256ll + threadIdx.x;
  if (q >= nquad) return;
  const int qw = g.Wp >> 2;
  const long long row = q / qw;
  const int xp0 = static_cast<int>(q - row * qw) << 2;
  const int yp = static_cast<int>(row % g.Hp);
  const long long img = row / g.Hp;
  const long long b = img >> 1;
  const unsigned char* src = ((img & 1) ? right : left) + b * g.H * g.W * g.C;
  const int ys = min(max(yp - g.top, 0), g.Hs - 1);
  const int c1 = g.C == 1 ? 0 : 1, c2 = g.C == 1 ? 0 : 2;        // gray replicates; alpha is never read

  RowTaps rt;
  if (RESIZE) {
    int y0, y1;
    taps(ys, g.H, g.scale, y0, y1, rt.wy);
    rt.r0 = src + static_cast<long long>(y0) * g.W * g.C;
    rt.r1 = src + static_cast<long long>(y1) * g.W * g.C;
  } else {
    rt.r0 = rt.r1 = src + static_cast<long long>(ys) * g.W * g.C;
    rt.wy = 0.f;
  }
  float v[3][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xs = min(max(xp0 + k - g.left, 0), g.Ws - 1);
    if (RESIZE) {
      int x0, x1;
      float wx;
      taps(xs, g.W, g.scale, x0, x1, wx);
      const unsigned char *a = rt.r0 + x0 * g.C, *bq = rt.r0 + x1 * g.C, *c = rt.r1 + x0 * g.C, *d = rt.r1 + x1 * g.C;
      v[0][k] = blend(a[0], bq[0], c[0], d[0], wx, rt.wy);
      v[1][k] = blend(a[c1], bq[c1], c[c1], d[c1], wx, rt.wy);
      v[2][k] = blend(a[c2], bq[c2], c[c2], d[c2], wx, rt.wy);
    } else {
      const unsigned char* a = rt.r0 + xs * g.C;
      v[0][k] = a[0];
      v[1][k] = a[c1];
      v[2][k] = a[c2];
    }
  }
  const long long plane = static_cast<long long>(g.Hp) * g.Wp;
  float* o = out + img * 3 * plane + static_cast<long long>(yp) * g.Wp + xp0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
  if (u8 && !(img & 1) && yp >= g.top && yp < g.top + g.Hs) {
    unsigned char* urow = u8 + (b * g.Hs + (yp - g.top)) * g.Ws * 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xs = xp0 + k - g.left;
      if (xs >= 0 && xs < g.Ws) {
        urow[3 * xs] = static_cast<unsigned char>(v[0][k]);
        urow[3 * xs + 1] = static_cast<unsigned char>(v[1][k]);
        urow[3 * xs + 2] = static_cast<unsigned char>(v[2][k]);
      }
    }
  }
}

// ---- min / max of the valid disparities -------------------------------------
__device__ __forceinline__ bool valid_disp(float d, float thres) { return !(d != d) && !(d >= thres); }

// Integer atomics on the bit pattern of a float: non-negative floats order as signed integers,
// negative floats in reverse as unsigned ones, so the pair below orders every non-NaN float as the
// reals do.  -0 is folded into +0 first (its pattern is the smallest signed integer).  min and max
// are exact and order-independent: the result does not depend on the arrival order of the blocks.
__device__ __forceinline__ void atomic_min_float(float* addr, float v) {
  v += 0.f;
  if (v >= 0.f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
  v += 0.f;
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

__global__ void minmax_init_kernel(float* __restrict__ minmax, int B) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < 2 * B) minmax[i] = (i & 1) ? -INFINITY : INFINITY;
}

// grid (blocks, B): the blocks of one image stride over its quads.  An image starts at b * P floats,
// 16-byte aligned only when that is a multiple of 4: up to 3 head pixels and P' % 4 tail pixels are
// read one by one, everything between them as float4.
__global__ __launch_bounds__(256) void disp_minmax_kernel(const float* __restrict__ disp, float* __restrict__ minmax,
                                                          long long P, float thres) {
  const int b = blockIdx.y;
  const long long start = b * P;
  const float* p = disp + start;
  const long long head = min(P, static_cast<long long>((4 - (start & 3)) & 3));
  const long long nquad = (P - head) >> 2;
  const long long tail = head + (nquad << 2);
  const long long t = blockIdx.x * 256ll + threadIdx.x, stride = gridDim.x * 256ll;
  float mn = INFINITY, mx = -INFINITY;
  auto take = [&](float d) {
    if (valid_disp(d, thres)) {
      mn = fminf(mn, d);
      mx = fmaxf(mx, d);
    }
  };
  if (t < head) take(p[t]);
  for (long long q = t; q < nquad; q += stride) {
    const float4 d = *reinterpret_cast<const float4*>(p + head + (q << 2));
    take(d.x); take(d.y); take(d.z); take(d.w);
  }
  if (tail + t < P) take(p[tail + t]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_down(mn, off, 64));
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
  }
  __shared__ float smn[4], smx[4];
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    if (mn <= mx) {                                         // the block saw a valid pixel
      atomic_min_float(minmax + 2 * b, mn);
      atomic_max_float(minmax + 2 * b + 1, mx);
    }
  }
}

// ---- the picture --------------------------------------------------------------
struct Picture {
  int H, W;
  long long P;            // B * H * W
  float thres;
  int side_by_side;       // image given: the row is [image | colours], 2W pixels
};

// Utils.py:126-133 for one pixel: LUT index, or -1 for an invalid pixel (black)
__device__ __forceinline__ int lut_index(float d, float mn, float mx, float thres) {
#pragma clang fp contract(off)
  if (!valid_disp(d, thres)) return -1;
  if (mx == mn) return 0;
  const float t = fminf(fmaxf((d - mn) / (mx - mn), 0.f), 1.f) * 255.f;
  return static_cast<int>(static_cast<unsigned char>(t));
}

// One lane owns 4 consecutive pixels of the flat (B,H,W) index: one float4 load, 12 output bytes.
// Without an image the 12 bytes sit at 12 q of the output: three 32-bit stores.  With one, a pixel
// of row r lands at pixel (r * 2W + W + col) and the quad may run over a row end, so the bytes go out
// one by one and the 12 image bytes beside them.  The thread after the last quad takes the P % 4
// pixels left.  The 768-byte LUT is staged in LDS once per block.
__global__ __launch_bounds__(256) void disp_colorize_kernel(const float* __restrict__ disp,
                                                            const float* __restrict__ minmax,
                                                            const unsigned char* __restrict__ lut,
                                                            const unsigned char* __restrict__ image,
                                                            unsigned char* __restrict__ out, Picture g) {
  __shared__ unsigned char slut[768];
  for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
  __syncthreads();
  const long long q = blockIdx.x * 256ll + threadIdx.x;
  const long long nquad = g.P >> 2;
  if (q > nquad) return;
  const long long p0 = q << 2;
  const int n = q < nquad ? 4 : static_cast<int>(g.P - p0);
  if (n == 0) return;
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (n == 4) {
    const float4 d4 = *reinterpret_cast<const float4*>(disp + p0);
    d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
  } else {
    for (int k = 0; k < n; ++k) d[k] = disp[p0 + k];
  }
  long long row = p0 / g.W;                                 // row of the flat (B*H, W) picture
  int col = static_cast<int>(p0 - row * g.W);
  unsigned char rgb[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long rk = row + (col + k) / g.W;             // col + k < 2W only if W > 3; divide to be safe
    const long long b = rk / g.H;
    const int idx = k < n ? lut_index(d[k], minmax[2 * b], minmax[2 * b + 1], g.thres) : -1;
    rgb[3 * k] = idx < 0 ? 0 : slut[3 * idx];
    rgb[3 * k + 1] = idx < 0 ? 0 : slut[3 * idx + 1];
    rgb[3 * k + 2] = idx < 0 ? 0 : slut[3 * idx + 2];
  }
  if (!g.side_by_side) {
    if (n == 4) {
      unsigned* o = reinterpret_cast<unsigned*>(out + 3 * p0);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        o[j] = rgb[4 * j] | (rgb[4 * j + 1] << 8) | (rgb[4 * j + 2] << 16) | (static_cast<unsigned>(rgb[4 * j + 3]) << 24);
    } else {
      for (int k = 0; k < 3 * n; ++k) out[3 * p0 + k] = rgb[k];
    }
  } else {
    for (int k = 0; k < n; ++k) {
      unsigned char* o = out + (row * 2 * g.W + col) * 3;
      const unsigned char* im = image + (p0 + k) * 3;
      o[0] = im[0]; o[1] = im[1]; o[2] = im[2];
      o += 3 * static_cast<long long>(g.W);
      o[0] = rgb[3 * k]; o[1] = rgb[3 * k + 1]; o[2] = rgb[3 * k + 2];
      if (++col == g.W) {
        col = 0;
        ++row;
      }
    }
  }
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" {

int fsmi_frames_ingest(const unsigned char* left, const unsigned char* right, float* out, unsigned char* image_u8,
                       int B, int H, int W, int C, double scale, int Hs, int Ws, int pad_left, int pad_right,
                       int pad_top, int pad_bottom, int divis_by, void* stream) {
  FSMI_CHECK_ARG(B > 0 && H > 0 && W > 0, "fsmi_frames_ingest: bad shape (%d,%d,%d)", B, H, W);
  FSMI_CHECK_ARG(C == 1 || C == 3 || C == 4, "fsmi_frames_ingest: C = %d: 1 (gray), 3 (RGB) or 4 (RGBA)", C);
  FSMI_CHECK_ARG(scale > 0.0 && scale <= 1.0, "fsmi_frames_ingest: scale = %g must be in (0, 1]", scale);
  FSMI_CHECK_ARG(Hs > 0 && Ws > 0 && Hs <= H && Ws <= W, "fsmi_frames_ingest: resized size (%d,%d) of (%d,%d)", Hs, Ws,
                 H, W);
  FSMI_CHECK_ARG(scale != 1.0 || (Hs == H && Ws == W), "fsmi_frames_ingest: scale 1 but resized size (%d,%d) != (%d,%d)",
                 Hs, Ws, H, W);
  FSMI_CHECK_ARG(pad_left >= 0 && pad_right >= 0 && pad_top >= 0 && pad_bottom >= 0, "fsmi_frames_ingest: negative pad");
  FSMI_CHECK_ARG(divis_by > 0, "fsmi_frames_ingest: divis_by = %d", divis_by);
  const long long Hp = static_cast<long long>(Hs) + pad_top + pad_bottom;
  const long long Wp = static_cast<long long>(Ws) + pad_left + pad_right;
  FSMI_CHECK_ARG(Hp % divis_by == 0 && Wp % divis_by == 0,
                 "fsmi_frames_ingest: padded size (%lld,%lld): Hp %% divis_by and Wp %% divis_by must be 0 (divis_by %d)",
                 Hp, Wp, divis_by);
  FSMI_CHECK_ARG(Wp % 4 == 0, "fsmi_frames_ingest: padded width %lld must be a multiple of 4", Wp);
  FSMI_CHECK_ARG(static_cast<long long>(H) * W * C <= INT_MAX && Hp * Wp <= INT_MAX,
                 "fsmi_frames_ingest: a frame exceeds 2^31 - 1 elements");
  FSMI_CHECK_ARG(left && right && out, "fsmi_frames_ingest: null pointer");
  FSMI_CHECK_ARG(aligned(out, 16), "fsmi_frames_ingest: out must be 16-byte aligned");
  const long long nquad = 2ll * B * Hp * (Wp >> 2);
  FSMI_CHECK_ARG((nquad + 255) / 256 <= INT_MAX, "fsmi_frames_ingest: too many pixels");
  Ingest g{H, W, C, Hs, Ws, static_cast<int>(Hp), static_cast<int>(Wp), pad_top, pad_left, scale};
  const dim3 grid(ceil_div(nquad, 256));
  if (scale == 1.0)
    hipLaunchKernelGGL(frames_ingest_kernel<false>, grid, dim3(256), 0, as_stream(stream), left, right, out, image_u8,
                       nquad, g);
  else
    hipLaunchKernelGGL(frames_ingest_kernel<true>, grid, dim3(256), 0, as_stream(stream), left, right, out, image_u8,
                       nquad, g);
  return finish_launch("fsmi_frames_ingest");
}

int fsmi_disp_minmax(const float* disp, float* minmax, int B, int H, int W, float invalid_thres, void* stream) {
  FSMI_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0, "fsmi_disp_minmax: bad shape (%d,%d,%d)", B, H, W);
  FSMI_CHECK_ARG(!std::isnan(invalid_thres), "fsmi_disp_minmax: invalid_thres is NaN");
  FSMI_CHECK_ARG(disp && minmax, "fsmi_disp_minmax: null pointer");
  FSMI_CHECK_ARG(aligned(disp, 16) && aligned(minmax, 4), "fsmi_disp_minmax: disp must be 16-byte aligned");
  const long long P = static_cast<long long>(H) * W;
  hipLaunchKernelGGL(minmax_init_kernel, dim3(ceil_div(2ll * B, 64)), dim3(64), 0, as_stream(stream), minmax, B);
  const unsigned blocks = std::min(ceil_div(ceil_div(P, 4), 256), 256u);
  hipLaunchKernelGGL(disp_minmax_kernel, dim3(blocks, B), dim3(256), 0, as_stream(stream), disp, minmax, P,
                     invalid_thres);
  return finish_launch("fsmi_disp_minmax");
}

int fsmi_disp_colorize(const float* disp, const float* minmax, const unsigned char* lut, const unsigned char* image,
                       unsigned char* out, int B, int H, int W, float invalid_thres, void* stream) {
  FSMI_CHECK_ARG(B > 0 && H > 0 && W > 0, "fsmi_disp_colorize: bad shape (%d,%d,%d)", B, H, W);
  const long long P = static_cast<long long>(B) * H * W;
  FSMI_CHECK_ARG(P <= INT_MAX / 6, "fsmi_disp_colorize: B*H*W = %lld exceeds (2^31 - 1) / 6", P);
  FSMI_CHECK_ARG(!std::isnan(invalid_thres), "fsmi_disp_colorize: invalid_thres is NaN");
  FSMI_CHECK_ARG(disp && minmax && lut && out, "fsmi_disp_colorize: null pointer");
  FSMI_CHECK_ARG(aligned(disp, 16) && aligned(out, 4), "fsmi_disp_colorize: disp must be 16-byte and out 4-byte aligned");
  Picture g{H, W, P, invalid_thres, image != nullptr};
  const long long nthreads = (P >> 2) + ((P & 3) ? 1 : 0);
  hipLaunchKernelGGL(disp_colorize_kernel, dim3(ceil_div(nthreads, 256)), dim3(256), 0, as_stream(stream), disp, minmax,
                     lut, image, out, g);
  return finish_launch("fsmi_disp_colorize");
}

}  // extern "C"
