// Does a disparity explain the two images?  The right frame warped into the left view, its residual
// (absolute difference, 3x3 SSIM) and the same absolute difference with the right frame sampled a few
// rows up and down (include/fsmi.h has the contract and every operation's order).
//   photo_tile      grid (tiles, B), one 64 x 12 tile of one pair per 256-thread block, two phases:
//     warp    every pixel of the tile and, with SSIM, of a one-pixel halo around it: disparity and left
//             pixel in (16 B per lane on the column quads whose row address allows it), its class, the
//             bilinear tap of the right row; left, warped, xr and the class go to LDS.  Each warped
//             value is computed once here and shared by the up to nine windows that hold it.
//     score   the tile's own pixels from LDS: warped / l1 / dssim maps out, the row probe's taps, and
//             the block's sums (block_reduce of metrics_common.h): one row of doubles STORED to the workspace
//   photo_finalize  one block per pair adds the tiles' rows in index order and writes sums and table
// The right image is gathered from global memory: a row's taps land on u - d, next to their
// neighbours', so a wave's taps of one row share cache lines and the rows of a tile stay in L2.
#include <climits>
#include <cstdint>

#include "metrics_common.h"

namespace fsmi {
namespace {

constexpr int kThreads = 256;
constexpr int TW = 64, TH = 12;           // tile: 16 column quads x 12 rows; with the halo 18 x 14 = 252 items
constexpr int RW = TW + 8, RH = TH + 2;   // LDS region: the halo column sits in a quad of its own on either side
constexpr int NFIX = FSMI_PHOTO_NFIXED;   // 8
constexpr int MAXOFF = FSMI_PHOTO_MAX_OFFSETS;
constexpr int NACC_MAX = NFIX + 2 * MAXOFF;
constexpr int kMaxBlocksY = 65535;

static_assert(NFIX == 8 && MAXOFF == 8, "accumulator layout: 8 fixed slots then (n, sum) per offset");
static_assert((TW & 3) == 0 && (RW & 3) == 0, "LDS rows are whole quads");

enum { A_SCORED = 0, A_SSIM, A_INVALID, A_OOV, A_L1, A_L1SQ, A_DS, A_L1S };
enum { CLS_INVALID = 0, CLS_OOV = 1, CLS_SAMPLED = 2 };

struct Params {
  int H, W, tiles_x, n_offsets;
  long long disp_bs, disp_rs;
  long long l_bs, l_cs, l_rs, r_bs, r_cs, r_rs;     // elements; the u8 format: (H*W*C, 1, W*C)
  float dy[MAXOFF];
};

// element i of an image row as a grey level
template <int FMT>
__device__ __forceinline__ float px(const void* base, long long i) {
  if constexpr (FMT == FSMI_IMAGE_U8_HWC) return static_cast<float>(static_cast<const unsigned char*>(base)[i]);
  else return static_cast<const float*>(base)[i];
}

// h(y) of fsmi.h for one channel: row points at R[b][c][y][0]
template <int FMT, int C>
__device__ __forceinline__ float tap(const void* img, long long row, int x0, int x1, float t) {
#pragma clang fp contract(off)
  constexpr int PS = FMT == FSMI_IMAGE_U8_HWC ? C : 1;
  const float a = px<FMT>(img, row + static_cast<long long>(x0) * PS);
  if (t == 0.f) return a;
  return a + t * (px<FMT>(img, row + static_cast<long long>(x1) * PS) - a);
}

template <int FMT, int C, bool SSIM, bool PROBE>
__global__ __launch_bounds__(kThreads) void photo_tile_kernel(const float* __restrict__ disp,
                                                              const void* __restrict__ left,
                                                              const void* __restrict__ right,
                                                              const unsigned char* __restrict__ mask,
                                                              float* __restrict__ warped, float* __restrict__ l1map,
                                                              float* __restrict__ dsmap, double* __restrict__ partials,
                                                              Params p) {
  constexpr bool U8 = FMT == FSMI_IMAGE_U8_HWC;
  constexpr int HALO = SSIM ? 1 : 0;
  constexpr int NSLOT = TW / 4 + 2 * HALO, NROW = TH + 2 * HALO;
  constexpr int NACC = PROBE ? NACC_MAX : NFIX;
  __shared__ __attribute__((aligned(16))) float Ls[C][RH][RW];
  __shared__ __attribute__((aligned(16))) float Ws[C][RH][RW];
  __shared__ __attribute__((aligned(16))) float Xr[RH][RW];
  __shared__ __attribute__((aligned(16))) unsigned char Cls[RH][RW];
  __shared__ double red[4][NACC_MAX];

  const int H = p.H, W = p.W;
  const int b = blockIdx.y;
  const int tyi = blockIdx.x / p.tiles_x, txi = blockIdx.x - tyi * p.tiles_x;
  const int cx0 = txi * TW, cy0 = tyi * TH;
  const long long lb = b * p.l_bs, rb = b * p.r_bs;

  // ---- warp: LDS row lr holds image row cy0 - 1 + lr, LDS column lc image column cx0 - 4 + lc
  for (int i = threadIdx.x; i < NROW * NSLOT; i += kThreads) {
#pragma clang fp contract(off)
    const int rr = i / NSLOT, s = i - rr * NSLOT;
    const int v = cy0 - HALO + rr, u0 = cx0 - 4 * HALO + 4 * s;
    if (v < 0 || v >= H) continue;
    // the columns j of the quad that are inside the image and inside tile + halo
    int jlo = (HALO && s == 0) ? 3 : 0, jhi = (HALO && s == NSLOT - 1) ? 1 : 4;
    jlo = max(jlo, -u0);
    jhi = min(jhi, W - u0);
    if (jlo >= jhi) continue;
    const bool full = jlo == 0 && jhi == 4;
    const int lr = v - (cy0 - 1), lc0 = u0 - (cx0 - 4);

    float d[4] = {}, L[C][4] = {};
    const float* dp = disp + b * p.disp_bs + v * p.disp_rs + u0;
    if (full && aligned(dp, 16)) {
      const float4 q = *reinterpret_cast<const float4*>(dp);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j >= jlo && j < jhi) d[j] = dp[j];
    }
    if constexpr (U8) {
      const unsigned char* lp = static_cast<const unsigned char*>(left) + lb + v * p.l_rs + static_cast<long long>(u0) * C;
      if (full && aligned(lp, 4)) {
        if constexpr (C == 3) {
          unsigned px4[4][3];
          unpack_rgb4(*reinterpret_cast<const uint3*>(lp), px4);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) L[c][j] = px4[j][c];
        } else {
          const unsigned w = *reinterpret_cast<const unsigned*>(lp);
          L[0][0] = w & 255u; L[0][1] = (w >> 8) & 255u; L[0][2] = (w >> 16) & 255u; L[0][3] = w >> 24;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < C; ++c)
            if (j >= jlo && j < jhi) L[c][j] = lp[j * C + c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* lp = static_cast<const float*>(left) + lb + c * p.l_cs + v * p.l_rs + u0;
        if (full && aligned(lp, 16)) {
          const float4 q = *reinterpret_cast<const float4*>(lp);
          L[c][0] = q.x; L[c][1] = q.y; L[c][2] = q.z; L[c][3] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j >= jlo && j < jhi) L[c][j] = lp[j];
        }
      }
    }

    float w[C][4] = {}, xr[4] = {};
    unsigned char cls[4] = {};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < jlo || j >= jhi) continue;
      const float dj = d[j];
      if (!(isfinite(dj) && dj > 0.f)) { cls[j] = CLS_INVALID; continue; }
      const float x = static_cast<float>(u0 + j) - dj;
      if (x < 0.f) { cls[j] = CLS_OOV; continue; }
      cls[j] = CLS_SAMPLED;
      xr[j] = x;
      // 0 <= x <= u <= W - 1: x0 is in [0, W - 1]
      const float xf = floorf(x);
      const int x0 = static_cast<int>(xf), x1 = min(x0 + 1, W - 1);
      const float t = x - xf;
#pragma unroll
      for (int c = 0; c < C; ++c) w[c][j] = tap<FMT, C>(right, rb + c * p.r_cs + v * p.r_rs, x0, x1, t);
    }
    if (full) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        *reinterpret_cast<float4*>(&Ls[c][lr][lc0]) = make_float4(L[c][0], L[c][1], L[c][2], L[c][3]);
        *reinterpret_cast<float4*>(&Ws[c][lr][lc0]) = make_float4(w[c][0], w[c][1], w[c][2], w[c][3]);
      }
      *reinterpret_cast<float4*>(&Xr[lr][lc0]) = make_float4(xr[0], xr[1], xr[2], xr[3]);
      *reinterpret_cast<uchar4*>(&Cls[lr][lc0]) = make_uchar4(cls[0], cls[1], cls[2], cls[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < jlo || j >= jhi) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) { Ls[c][lr][lc0 + j] = L[c][j]; Ws[c][lr][lc0 + j] = w[c][j]; }
        Xr[lr][lc0 + j] = xr[j];
        Cls[lr][lc0 + j] = cls[j];
      }
    }
  }
  __syncthreads();

  // ---- score: the tile's own pixels
  unsigned n_scored = 0, n_ssim = 0, n_invalid = 0, n_oov = 0, n_r[MAXOFF] = {};
  double s_l1 = 0.0, s_l1sq = 0.0, s_ds = 0.0, s_l1s = 0.0, s_r[MAXOFF] = {};
  for (int i = threadIdx.x; i < TH * (TW / 4); i += kThreads) {
#pragma clang fp contract(off)
    const int rr = i / (TW / 4), s = i - rr * (TW / 4);
    const int v = cy0 + rr, u0 = cx0 + 4 * s;
    if (v >= H || u0 >= W) continue;
    const int n = min(4, W - u0);
    const int lr = rr + 1, lc0 = 4 * s + 4;
    const long long o = (static_cast<long long>(b) * H + v) * W + u0;      // the contiguous maps and the mask
    unsigned m4 = 0x01010101u;
    if (mask) {
      const unsigned char* mp = mask + o;
      if (n == 4 && aligned(mp, 4)) {
        m4 = *reinterpret_cast<const unsigned*>(mp);
      } else {
        m4 = 0;
        for (int j = 0; j < n; ++j) m4 |= static_cast<unsigned>(mp[j]) << (8 * j);
      }
    }
    float l1v[4], dsv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l1v[j] = INFINITY;
      dsv[j] = INFINITY;
      if (j >= n) continue;
      const int lc = lc0 + j, u = u0 + j;
      const int cls = Cls[lr][lc];
      n_invalid += cls == CLS_INVALID;
      n_oov += cls == CLS_OOV;
      const bool scored = cls == CLS_SAMPLED && ((m4 >> (8 * j)) & 255u) != 0;
      if (!scored) continue;
      float l1 = fabsf(Ls[0][lr][lc] - Ws[0][lr][lc]);
      if constexpr (C == 3) {
        l1 = ((l1 + fabsf(Ls[1][lr][lc] - Ws[1][lr][lc])) + fabsf(Ls[2][lr][lc] - Ws[2][lr][lc])) / 3.0f;
      }
      l1v[j] = l1;
      const double l1d = static_cast<double>(l1);
      n_scored += 1;
      s_l1 += l1d;
      s_l1sq += l1d * l1d;

      if constexpr (PROBE) {
        const float x = Xr[lr][lc];
        const float xf = floorf(x);
        const int x0 = static_cast<int>(xf), x1 = min(x0 + 1, W - 1);
        const float t = x - xf;
#pragma unroll
        for (int k = 0; k < MAXOFF; ++k) {
          if (k >= p.n_offsets) continue;
          const float yr = static_cast<float>(v) + p.dy[k];
          if (!(yr >= 0.f && yr <= static_cast<float>(H - 1))) continue;
          const float yf = floorf(yr);
          const int y0 = static_cast<int>(yf), y1 = min(y0 + 1, H - 1);
          const float ty = yr - yf;
          float e = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const long long base = rb + c * p.r_cs;
            const float h0 = tap<FMT, C>(right, base + y0 * p.r_rs, x0, x1, t);
            float wv = h0;
            if (ty != 0.f) wv = h0 + ty * (tap<FMT, C>(right, base + y1 * p.r_rs, x0, x1, t) - h0);
            const float a = fabsf(Ls[c][lr][lc] - wv);
            e = c == 0 ? a : e + a;
          }
          if constexpr (C == 3) e = e / 3.0f;
          n_r[k] += 1;
          s_r[k] += static_cast<double>(e);
        }
      }

      if constexpr (SSIM) {
        if (u < 1 || u > W - 2 || v < 1 || v > H - 2) continue;
        bool all = true;
#pragma unroll
        for (int a = -1; a <= 1; ++a)
#pragma unroll
          for (int c = -1; c <= 1; ++c) all = all && Cls[lr + a][lc + c] == CLS_SAMPLED;
        if (!all) continue;
        float ds = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float xs[9], ys[9];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              xs[3 * a + q] = Ls[c][lr - 1 + a][lc - 1 + q];
              ys[3 * a + q] = Ws[c][lr - 1 + a][lc - 1 + q];
            }
          float sx = xs[0], sy = ys[0];
#pragma unroll
          for (int k = 1; k < 9; ++k) { sx = sx + xs[k]; sy = sy + ys[k]; }
          const float mx = sx / 9.0f, my = sy / 9.0f;
          float vx = 0.f, vy = 0.f, cxy = 0.f;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            const float ex = xs[k] - mx, ey = ys[k] - my;
            const float pxx = ex * ex, pyy = ey * ey, pxy = ex * ey;
            vx = k == 0 ? pxx : vx + pxx;
            vy = k == 0 ? pyy : vy + pyy;
            cxy = k == 0 ? pxy : cxy + pxy;
          }
          vx = vx / 9.0f; vy = vy / 9.0f; cxy = cxy / 9.0f;
          const float num = ((2.0f * mx) * my + 6.5025f) * (2.0f * cxy + 58.5225f);
          const float den = ((mx * mx + my * my) + 6.5025f) * ((vx + vy) + 58.5225f);
          float dc = (1.0f - num / den) * 0.5f;
          if (!(dc >= 0.f)) dc = 0.f;
          if (dc > 1.f) dc = 1.f;
          ds = c == 0 ? dc : ds + dc;
        }
        if constexpr (C == 3) ds = ds / 3.0f;
        dsv[j] = ds;
        n_ssim += 1;
        s_ds += static_cast<double>(ds);
        s_l1s += l1d;
      }
    }
    const bool quad = n == 4;
    if (warped) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float* wp = warped + ((static_cast<long long>(b) * C + c) * H + v) * W + u0;
        if (quad && aligned(wp, 16)) {
          *reinterpret_cast<float4*>(wp) = *reinterpret_cast<const float4*>(&Ws[c][lr][lc0]);
        } else {
          for (int j = 0; j < n; ++j) wp[j] = Ws[c][lr][lc0 + j];
        }
      }
    }
    if (l1map) {
      float* q = l1map + o;
      if (quad && aligned(q, 16)) *reinterpret_cast<float4*>(q) = make_float4(l1v[0], l1v[1], l1v[2], l1v[3]);
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < n) q[j] = l1v[j];
      }
    }
    if (SSIM && dsmap) {
      float* q = dsmap + o;
      if (quad && aligned(q, 16)) *reinterpret_cast<float4*>(q) = make_float4(dsv[0], dsv[1], dsv[2], dsv[3]);
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < n) q[j] = dsv[j];
      }
    }
  }

  double acc[NACC];
  acc[A_SCORED] = n_scored; acc[A_SSIM] = n_ssim; acc[A_INVALID] = n_invalid; acc[A_OOV] = n_oov;
  acc[A_L1] = s_l1; acc[A_L1SQ] = s_l1sq; acc[A_DS] = s_ds; acc[A_L1S] = s_l1s;
  if constexpr (PROBE) {
#pragma unroll
    for (int k = 0; k < MAXOFF; ++k) { acc[NFIX + 2 * k] = n_r[k]; acc[NFIX + 2 * k + 1] = s_r[k]; }
  }
  const double r = block_reduce<NACC>(acc, red);
  const int nt = NFIX + 2 * p.n_offsets;
  if (static_cast<int>(threadIdx.x) < nt)       // nt <= NACC: without PROBE n_offsets is 0
    partials[(static_cast<long long>(b) * gridDim.x + blockIdx.x) * nt + threadIdx.x] = r;
}

// One block per pair.  Lane t adds the rows t, t + 256, ... of the pair's NB tile rows in index order,
// then the same block_reduce; lane 0 turns the sums into the table.
__global__ __launch_bounds__(kThreads) void photo_finalize_kernel(const double* __restrict__ partials,
                                                                  double* __restrict__ sums, double* __restrict__ table,
                                                                  long long NB, int n_offsets, double alpha) {
#pragma clang fp contract(off)
  __shared__ double red[4][NACC_MAX];
  __shared__ double row[NACC_MAX];
  const int b = blockIdx.x;
  const int nt = NFIX + 2 * n_offsets;
  double v[NACC_MAX];
#pragma unroll
  for (int s = 0; s < NACC_MAX; ++s) v[s] = 0.0;
  for (long long r = threadIdx.x; r < NB; r += kThreads) {
    const double* src = partials + (b * NB + r) * nt;
#pragma unroll
    for (int s = 0; s < NACC_MAX; ++s)
      if (s < nt) v[s] += src[s];
  }
  const double r = block_reduce<NACC_MAX>(v, red);
  if (static_cast<int>(threadIdx.x) < nt) {
    sums[static_cast<long long>(b) * nt + threadIdx.x] = r;
    row[threadIdx.x] = r;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* o = table + static_cast<long long>(b) * nt;
  const double n = row[A_SCORED], ns = row[A_SSIM];
  o[0] = n; o[1] = ns; o[2] = row[A_INVALID]; o[3] = row[A_OOV];
  o[4] = n > 0.0 ? row[A_L1] / n : 0.0;
  o[5] = n > 0.0 ? sqrt(row[A_L1SQ] / n) : 0.0;
  o[6] = ns > 0.0 ? row[A_DS] / ns : 0.0;
  o[7] = ns > 0.0 ? (alpha * row[A_DS] + ((1.0 - alpha) * row[A_L1S]) / 255.0) / ns : 0.0;
  for (int k = 0; k < n_offsets; ++k) {
    const double nr = row[NFIX + 2 * k];
    o[NFIX + 2 * k] = nr;
    o[NFIX + 2 * k + 1] = nr > 0.0 ? row[NFIX + 2 * k + 1] / nr : 0.0;
  }
}

inline long long tiles_of(int H, int W, int* tiles_x) {
  const long long tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH;
  if (tiles_x) *tiles_x = static_cast<int>(tx);
  return tx * ty;
}

template <int FMT, int C, bool SSIM>
void launch(bool probe, dim3 grid, hipStream_t s, const float* disp, const void* left, const void* right,
            const unsigned char* mask, float* warped, float* l1, float* dssim, double* ws, const Params& p) {
  if (probe)
    hipLaunchKernelGGL((photo_tile_kernel<FMT, C, SSIM, true>), grid, dim3(kThreads), 0, s, disp, left, right, mask,
                       warped, l1, dssim, ws, p);
  else
    hipLaunchKernelGGL((photo_tile_kernel<FMT, C, SSIM, false>), grid, dim3(kThreads), 0, s, disp, left, right, mask,
                       warped, l1, dssim, ws, p);
}

template <int FMT, int C>
void launch(bool ssim, bool probe, dim3 grid, hipStream_t s, const float* disp, const void* left, const void* right,
            const unsigned char* mask, float* warped, float* l1, float* dssim, double* ws, const Params& p) {
  if (ssim) launch<FMT, C, true>(probe, grid, s, disp, left, right, mask, warped, l1, dssim, ws, p);
  else launch<FMT, C, false>(probe, grid, s, disp, left, right, mask, warped, l1, dssim, ws, p);
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" {

size_t fsmi_photo_consistency_ws_bytes(int B, int H, int W, int n_offsets) {
  if (B < 1 || H < 1 || W < 1 || n_offsets < 0 || n_offsets > MAXOFF) return 0;
  return static_cast<size_t>(B) * static_cast<size_t>(tiles_of(H, W, nullptr)) * (NFIX + 2 * n_offsets) * sizeof(double);
}

int fsmi_photo_consistency(const float* disp, const void* left, const void* right, const unsigned char* mask_or_null,
                           float* warped_or_null, float* l1_or_null, float* dssim_or_null, double* table, double* sums,
                           double* workspace, int B, int C, int H, int W, int image_format, long long disp_batch_stride,
                           long long disp_row_stride, long long left_batch_stride, long long left_channel_stride,
                           long long left_row_stride, long long right_batch_stride, long long right_channel_stride,
                           long long right_row_stride, const float* row_offsets, int n_offsets, double alpha, int ssim,
                           void* stream) {
  FSMI_CHECK_ARG(B >= 1 && B <= kMaxBlocksY && H >= 1 && W >= 1, "fsmi_photo_consistency: bad shape (%d,%d,%d)", B, H, W);
  FSMI_CHECK_ARG(C == 1 || C == 3, "fsmi_photo_consistency: C = %d channels: 1 or 3", C);
  FSMI_CHECK_ARG(image_format == FSMI_IMAGE_F32_PLANAR || image_format == FSMI_IMAGE_U8_HWC,
                 "fsmi_photo_consistency: image_format = %d: FSMI_IMAGE_F32_PLANAR or FSMI_IMAGE_U8_HWC", image_format);
  FSMI_CHECK_ARG(static_cast<long long>(H) * W <= INT_MAX, "fsmi_photo_consistency: H*W = %lld exceeds 2^31 - 1",
                 static_cast<long long>(H) * W);
  FSMI_CHECK_ARG(n_offsets >= 0 && n_offsets <= MAXOFF, "fsmi_photo_consistency: n_offsets = %d row offsets: 0..%d",
                 n_offsets, MAXOFF);
  FSMI_CHECK_ARG(n_offsets == 0 || row_offsets, "fsmi_photo_consistency: null row_offsets with n_offsets = %d", n_offsets);
  for (int k = 0; k < n_offsets; ++k)
    FSMI_CHECK_ARG(std::isfinite(row_offsets[k]), "fsmi_photo_consistency: row offset %d is not finite", k);
  FSMI_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0, "fsmi_photo_consistency: alpha = %g must be in [0,1]", alpha);
  FSMI_CHECK_ARG(disp && left && right && table && sums && workspace, "fsmi_photo_consistency: null pointer");
  FSMI_CHECK_ARG(!dssim_or_null || ssim, "fsmi_photo_consistency: the dssim map needs ssim != 0");
  const bool u8 = image_format == FSMI_IMAGE_U8_HWC;
  FSMI_CHECK_ARG(aligned(warped_or_null, 16) && aligned(l1_or_null, 16) && aligned(dssim_or_null, 16),
                 "fsmi_photo_consistency: warped, l1 and dssim must be 16-byte aligned");
  FSMI_CHECK_ARG(aligned(disp, 4) && (u8 || (aligned(left, 4) && aligned(right, 4))) && aligned(table, 8) &&
                     aligned(sums, 8) && aligned(workspace, 8),
                 "fsmi_photo_consistency: fp32 inputs must be 4-byte aligned, fp64 outputs and the workspace 8-byte aligned");
  FSMI_CHECK_ARG(disp_row_stride >= W && disp_batch_stride >= 0,
                 "fsmi_photo_consistency: disp strides (%lld,%lld): the row stride must be at least W", disp_batch_stride,
                 disp_row_stride);
  FSMI_CHECK_ARG(u8 || (left_row_stride >= W && right_row_stride >= W && left_batch_stride >= 0 &&
                        right_batch_stride >= 0 && left_channel_stride >= 0 && right_channel_stride >= 0),
                 "fsmi_photo_consistency: image row strides must be at least W and no stride negative");
  Params p;
  p.H = H;
  p.W = W;
  p.n_offsets = n_offsets;
  const long long NB = tiles_of(H, W, &p.tiles_x);                 // <= H * W <= INT_MAX
  p.disp_bs = disp_batch_stride;
  p.disp_rs = disp_row_stride;
  if (u8) {
    p.l_bs = p.r_bs = static_cast<long long>(H) * W * C;
    p.l_cs = p.r_cs = 1;
    p.l_rs = p.r_rs = static_cast<long long>(W) * C;
  } else {
    p.l_bs = left_batch_stride; p.l_cs = left_channel_stride; p.l_rs = left_row_stride;
    p.r_bs = right_batch_stride; p.r_cs = right_channel_stride; p.r_rs = right_row_stride;
  }
  for (int k = 0; k < MAXOFF; ++k) p.dy[k] = k < n_offsets ? row_offsets[k] : 0.f;
  hipStream_t s = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(NB), static_cast<unsigned>(B));
  const bool probe = n_offsets > 0, with_ssim = ssim != 0;
#define FSMI_PHOTO_LAUNCH(FMT, CC) \
  launch<FMT, CC>(with_ssim, probe, grid, s, disp, left, right, mask_or_null, warped_or_null, l1_or_null, dssim_or_null, \
                  workspace, p)
  if (u8 && C == 3) FSMI_PHOTO_LAUNCH(FSMI_IMAGE_U8_HWC, 3);
  else if (u8) FSMI_PHOTO_LAUNCH(FSMI_IMAGE_U8_HWC, 1);
  else if (C == 3) FSMI_PHOTO_LAUNCH(FSMI_IMAGE_F32_PLANAR, 3);
  else FSMI_PHOTO_LAUNCH(FSMI_IMAGE_F32_PLANAR, 1);
#undef FSMI_PHOTO_LAUNCH
  hipLaunchKernelGGL(photo_finalize_kernel, dim3(B), dim3(kThreads), 0, s, workspace, sums, table, NB, n_offsets, alpha);
  return finish_launch("fsmi_photo_consistency");
}

}  // extern "C"
