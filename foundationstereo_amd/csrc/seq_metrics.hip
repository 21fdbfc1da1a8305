// Every refinement iteration scored in one pass: up to 64 prediction maps ("rows") of one batch against
// one ground truth, and the weighted sequence loss (train/losses.py:379-498 foundation_stereo_loss and
// the single-map losses :20-187, which gather through a boolean mask per map, resize with F.interpolate
// and synchronise the host about 7 times per map).  include/fsmi.h has the arithmetic and the layouts.
//   seq_metrics_partial   grid (NB, row groups, B): a block takes kRowsPerBlock rows of its launch and
//                         strides over 1024-pixel tiles of pair b; it loads a pixel's ground truth and
//                         mask once and reuses them for its rows, whose accumulators stay in registers;
//                         per row it STORES one partial row of 14 doubles (no float atomics)
//   seq_metrics_finalize  one block per pair, once per call: a wave per row adds that row's NB partial
//                         rows in index order and finishes with the shuffle tree; thread 0 then adds the
//                         weighted loss in row order
// Rows are strided views with 4-byte alignment only, so every load is one dword per lane (a wave reads
// 256 contiguous bytes of a line).  Row descriptors travel by value in the kernarg: 32 rows per launch.
#include <climits>
#include <cstdint>

#include "metrics_common.h"

namespace fsmi {
namespace {

constexpr int NACC = FSMI_SEQ_NACC;
constexpr int MAXT = FSMI_METRICS_MAX_THRESHOLDS;
constexpr int MAXR = FSMI_SEQ_MAX_ROWS;
constexpr int kRowsPerBlock = 4;          // rows whose accumulators a lane holds
constexpr int kRowsPerLaunch = 32;        // 32 descriptors of 56 bytes: well under the 4 KB kernarg
constexpr int kTile = 1024;               // pixels per block and step: 256 lanes x 4 pixels, 256 apart
constexpr int kMaxBlocks = 512;           // per pair; the finalize reads at most 8 partial rows per lane

static_assert(NACC == 6 + MAXT, "accumulator layout: 6 fixed slots then the thresholds");
static_assert(kRowsPerLaunch % kRowsPerBlock == 0 && MAXR % kRowsPerLaunch == 0, "row split");

enum { A_N = 0, A_SE, A_SE2, A_SL1, A_D1, A_NONFINITE, A_BAD };

struct SeqRow {
  const float* p;
  long long bs, rs;       // elements between pairs, between lines
  int h, w;
  float sy, sx;           // (float)h / (float)H, (float)w / (float)W
  float mul, maxd;
  int resize;             // (h, w) != (H, W)
};

struct SeqRows {
  SeqRow r[kRowsPerLaunch];
};

struct SeqParams {
  long long P;            // H * W
  double gt_scale;
  int W;
  int R, row0, nrows;     // rows of the call, first row and row count of this launch
  float beta;
  float thr[MAXT];        // unused slots +inf: e > +inf never counts
};

struct SeqLoss {
  double w[MAXR];
  unsigned long long smooth;   // bit r: row r enters the loss with its smooth-L1 mean, else its EPE
};

// One lane's running row.  Counts stay below 2^32 per lane (a pair has at most 2^31 - 1 pixels).
struct Lane {
  double se = 0.0, se2 = 0.0, sl1 = 0.0;
  unsigned n = 0, d1 = 0, nonfinite = 0, bad[MAXT] = {};
};

// F.interpolate(align_corners=False)'s source index along one axis
__device__ __forceinline__ void tap(float s, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  float src = s * (static_cast<float>(dst) + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min(static_cast<int>(src), in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = src - static_cast<float>(i0);
  l0 = 1.f - l1;
}

// the row's value at pixel (y, x) of the ground truth's grid, after the factor and the clamp
__device__ __forceinline__ float sample(const SeqRow& r, int b, int y, int x) {
#pragma clang fp contract(off)
  const float* p = r.p + b * r.bs;
  float v;
  if (r.resize) {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    tap(r.sy, y, r.h, y0, y1, ly0, ly1);
    tap(r.sx, x, r.w, x0, x1, lx0, lx1);
    const float* a = p + y0 * r.rs;
    const float* c = p + y1 * r.rs;
    const float p00 = a[x0], p01 = a[x1], p10 = c[x0], p11 = c[x1];
    v = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
  } else {
    v = p[y * r.rs + x];
  }
  v = v * r.mul;
  if (r.maxd < INFINITY) {                     // torch.clamp: the comparisons keep a NaN
    v = v < 0.f ? 0.f : v;
    v = v > r.maxd ? r.maxd : v;
  }
  return v;
}

__device__ __forceinline__ void take(Lane& a, float v, float gt, bool valid, const SeqParams& g) {
#pragma clang fp contract(off)
  const float e = fabsf(v - gt);
  const float beta = g.beta;
  const float s = beta == 0.f ? e : (e < beta ? __fdiv_rn(0.5f * (e * e), beta) : e - 0.5f * beta);
  const double ed = static_cast<double>(e);
  // an invalid pixel adds an exact 0.0 (never its NaN) and counts nowhere
  a.se += valid ? ed : 0.0;
  a.se2 += valid ? ed * ed : 0.0;
  a.sl1 += valid ? static_cast<double>(s) : 0.0;
  a.n += valid ? 1u : 0u;
  a.d1 += (valid && e > 3.0f && e > __fmul_rn(0.05f, fabsf(gt))) ? 1u : 0u;
  a.nonfinite += (valid && !(e < INFINITY)) ? 1u : 0u;                 // NaN or inf
#pragma unroll
  for (int k = 0; k < MAXT; ++k) a.bad[k] += (valid && e > g.thr[k]) ? 1u : 0u;
}

template <bool U8GT>
__global__ __launch_bounds__(256) void seq_metrics_partial_kernel(SeqRows rows, const void* __restrict__ gt_any,
                                                                  const unsigned char* __restrict__ mask,
                                                                  double* __restrict__ partials, SeqParams g) {
  __shared__ double lds[kRowsPerBlock][4][NACC];
  const int b = blockIdx.z;
  const int first = blockIdx.y * kRowsPerBlock;                       // within this launch
  const int nr = min(kRowsPerBlock, g.nrows - first);
  const long long P = g.P, start = b * P;
  const GroundTruth<U8GT> gts(gt_any, start, g.gt_scale);
  const unsigned char* mk = mask ? mask + start : nullptr;
  const bool has_mask = mask != nullptr;
  const unsigned W = static_cast<unsigned>(g.W);
  const long long ntiles = (P + kTile - 1) / kTile;

  Lane a[kRowsPerBlock];
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kTile / 256; ++j) {
      const long long i = tile * kTile + j * 256 + threadIdx.x;
      const bool inside = i < P;
      const unsigned ic = inside ? static_cast<unsigned>(i) : 0u;    // a lane past the end re-reads pixel 0
      const float gt = gts[ic];
      const bool valid = inside && pixel_valid(has_mask, has_mask ? mk[ic] : 0, gt);
      const unsigned y = ic / W, x = ic - y * W;
#pragma unroll
      for (int q = 0; q < kRowsPerBlock; ++q) {
        if (q < nr) take(a[q], sample(rows.r[first + q], b, static_cast<int>(y), static_cast<int>(x)), gt, valid, g);
      }
    }
  }

#pragma unroll
  for (int q = 0; q < kRowsPerBlock; ++q) {
    double v[NACC];
    v[A_N] = a[q].n; v[A_SE] = a[q].se; v[A_SE2] = a[q].se2; v[A_SL1] = a[q].sl1; v[A_D1] = a[q].d1;
    v[A_NONFINITE] = a[q].nonfinite;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) v[A_BAD + k] = a[q].bad[k];
    wave_reduce(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int s = 0; s < NACC; ++s) lds[q][threadIdx.x >> 6][s] = v[s];
    }
  }
  __syncthreads();
  if (threadIdx.x < nr * NACC) {                                       // waves 0..3 in index order
    const int q = threadIdx.x / NACC, s = threadIdx.x - q * NACC;
    const double r = ((lds[q][0][s] + lds[q][1][s]) + lds[q][2][s]) + lds[q][3][s];
    const long long row = static_cast<long long>(b) * g.R + g.row0 + first + q;
    partials[(row * gridDim.x + blockIdx.x) * NACC + s] = r;
  }
}

// One block per pair.  Wave w takes rows w, w + 4, ...: lane l adds partial rows l, l + 64, ... of the
// row in index order, then the shuffle tree; lane 0 writes the accumulators and the table.
__global__ __launch_bounds__(256) void seq_metrics_finalize_kernel(const double* __restrict__ partials,
                                                                   double* __restrict__ sums,
                                                                   double* __restrict__ table,
                                                                   double* __restrict__ loss, int NB, int R,
                                                                   SeqLoss L) {
#pragma clang fp contract(off)
  __shared__ double term[MAXR];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < R; r += 4) {
    const long long row = static_cast<long long>(b) * R + r;
    double v[NACC];
#pragma unroll
    for (int s = 0; s < NACC; ++s) v[s] = 0.0;
    for (int i = lane; i < NB; i += 64) {
      const double* src = partials + (row * NB + i) * NACC;
#pragma unroll
      for (int s = 0; s < NACC; ++s) v[s] += src[s];
    }
    wave_reduce(v);
    if (lane == 0) {
      double* o = sums + row * NACC;
      double* t = table + row * NACC;
      const double n = v[A_N];
      const bool any = n > 0.0;                                        // train/losses.py:60: an empty mask scores 0
      const double epe = any ? v[A_SE] / n : 0.0, sl1 = any ? v[A_SL1] / n : 0.0;
#pragma unroll
      for (int s = 0; s < NACC; ++s) o[s] = v[s];
      t[A_N] = n;
      t[A_SE] = epe;
      t[A_SE2] = any ? sqrt(v[A_SE2] / n) : 0.0;
      t[A_SL1] = sl1;
      t[A_D1] = any ? v[A_D1] / n : 0.0;
      t[A_NONFINITE] = v[A_NONFINITE];
#pragma unroll
      for (int k = 0; k < MAXT; ++k) t[A_BAD + k] = any ? v[A_BAD + k] / n : 0.0;
      term[r] = ((L.smooth >> r) & 1ull) ? sl1 : epe;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double acc = 0.0;
  for (int r = 0; r < R; ++r) acc = acc + L.w[r] * term[r];
  loss[b] = acc;
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" {

int fsmi_seq_metrics_blocks(int H, int W, int R) {
  if (H < 1 || W < 1 || R < 1) return 1;
  const long long tiles = (static_cast<long long>(H) * W + kTile - 1) / kTile;
  return static_cast<int>(std::min<long long>(std::max<long long>(tiles, 1), kMaxBlocks));
}

int fsmi_seq_metrics(const float* const* rows, const long long* batch_strides, const long long* row_strides,
                     const int* hs, const int* ws, const float* muls, const float* max_disps, const double* weights,
                     const unsigned char* smooth, int R, const float* gt, const unsigned char* gt_u8,
                     const unsigned char* mask, const float* thresholds, int K, double gt_scale, float beta,
                     double* partials, double* sums, double* table, double* loss, int B, int H, int W, void* stream) {
  float thr[MAXT];
  if (const int e = check_scoring_args("fsmi_seq_metrics", B, H, W, gt, gt_u8, gt_scale, thresholds, K, thr)) return e;
  FSMI_CHECK_ARG(R >= 1 && R <= MAXR, "fsmi_seq_metrics: R = %d rows: 1..%d", R, MAXR);
  FSMI_CHECK_ARG(beta >= 0.f, "fsmi_seq_metrics: beta = %g must not be negative", static_cast<double>(beta));
  FSMI_CHECK_ARG(rows && batch_strides && row_strides && hs && ws && muls && max_disps && weights && smooth &&
                     partials && sums && table && loss,
                 "fsmi_seq_metrics: null pointer");
  FSMI_CHECK_ARG((!gt || aligned(gt, 4)) && aligned(partials, 8) && aligned(sums, 8) && aligned(table, 8) &&
                     aligned(loss, 8),
                 "fsmi_seq_metrics: fp32 maps must be 4-byte and fp64 outputs 8-byte aligned");
  SeqLoss L;
  L.smooth = 0;
  for (int r = 0; r < MAXR; ++r) L.w[r] = 0.0;
  for (int r = 0; r < R; ++r) {
    FSMI_CHECK_ARG(rows[r] && aligned(rows[r], 4), "fsmi_seq_metrics: row %d: null or not 4-byte aligned", r);
    FSMI_CHECK_ARG(hs[r] >= 1 && ws[r] >= 1, "fsmi_seq_metrics: row %d: bad shape (%d,%d)", r, hs[r], ws[r]);
    FSMI_CHECK_ARG(row_strides[r] >= ws[r], "fsmi_seq_metrics: row %d: row stride %lld below its width %d", r,
                   row_strides[r], ws[r]);
    FSMI_CHECK_ARG(batch_strides[r] >= 0, "fsmi_seq_metrics: row %d: negative batch stride %lld", r, batch_strides[r]);
    FSMI_CHECK_ARG(!(max_disps[r] != max_disps[r]), "fsmi_seq_metrics: row %d: max_disp is NaN", r);
    L.w[r] = weights[r];
    if (smooth[r]) L.smooth |= 1ull << r;
  }
  const int NB = fsmi_seq_metrics_blocks(H, W, R);
  hipStream_t s = as_stream(stream);
  for (int row0 = 0; row0 < R; row0 += kRowsPerLaunch) {
    SeqRows d;
    SeqParams g;
    g.P = static_cast<long long>(H) * W;
    g.gt_scale = gt_scale;
    g.W = W;
    g.R = R;
    g.row0 = row0;
    g.nrows = std::min(kRowsPerLaunch, R - row0);
    g.beta = beta;
    std::copy(thr, thr + MAXT, g.thr);
    for (int q = 0; q < kRowsPerLaunch; ++q) {
      const int r = row0 + std::min(q, g.nrows - 1);                   // unused slots repeat the last row; never read
      SeqRow& o = d.r[q];
      o.p = rows[r];
      o.bs = batch_strides[r];
      o.rs = row_strides[r];
      o.h = hs[r];
      o.w = ws[r];
      o.sy = static_cast<float>(hs[r]) / static_cast<float>(H);
      o.sx = static_cast<float>(ws[r]) / static_cast<float>(W);
      o.mul = muls[r];
      o.maxd = max_disps[r];
      o.resize = (hs[r] != H || ws[r] != W) ? 1 : 0;
    }
    const dim3 grid(NB, ceil_div(g.nrows, kRowsPerBlock), B);
    if (gt_u8)
      hipLaunchKernelGGL(seq_metrics_partial_kernel<true>, grid, dim3(256), 0, s, d, static_cast<const void*>(gt_u8),
                         mask, partials, g);
    else
      hipLaunchKernelGGL(seq_metrics_partial_kernel<false>, grid, dim3(256), 0, s, d, static_cast<const void*>(gt), mask,
                         partials, g);
  }
  hipLaunchKernelGGL(seq_metrics_finalize_kernel, dim3(B), dim3(256), 0, s, partials, sums, table, loss, NB, R, L);
  return finish_launch("fsmi_seq_metrics");
}

}  // extern "C"
