// The histogram behind the sparsification (risk-coverage) curve (include/fsmi.h has the contract):
// pixels binned by confidence, per bin the pixel count and the sum of |pred - gt| in units of 2^-20 px.
// Every sum is an integer, so the result does not depend on the order of the additions and integer
// atomics are safe: a workgroup keeps a (count u32, sum u64) histogram in LDS while it strides over the
// pixels of one pair, then adds its non-empty bins to the pair's rows with one 64-bit atomic each.
#include <climits>

#include "metrics_common.h"

namespace fsmi {
namespace {

constexpr int kThreads = 256;
constexpr int kPixelsPerBlock = 8192;     // 32 per lane before a pair gets a second workgroup
constexpr int kMaxBlocks = 1024;          // 256 CUs x 4; beyond it a workgroup takes more pixels
constexpr int kBatch = 4;                 // loads in flight per lane and map

struct Params {
  const float* conf;                      // null: the oracle ranking
  const float* pred;
  const float* gt;
  const unsigned char* mask;
  unsigned long long* count;
  unsigned long long* err_q20;
  unsigned long long* dropped;
  long long P;                            // H * W
  int nbins, blocks_per_pair;
  float err_bin_scale;
};

__global__ __launch_bounds__(kThreads) void risk_coverage_kernel(Params p) {
  extern __shared__ unsigned long long lds[];                      // [nbins] sums, then [nbins] counts, then dropped
  unsigned long long* sum = lds;
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lds + p.nbins);
  unsigned int* drop = cnt + p.nbins;
  for (int k = threadIdx.x; k < p.nbins; k += kThreads) { sum[k] = 0ull; cnt[k] = 0u; }
  if (threadIdx.x == 0) *drop = 0u;
  __syncthreads();

  const int b = blockIdx.x / p.blocks_per_pair;
  const long long start = b * p.P;
  const float* conf = p.conf ? p.conf + start : nullptr;
  const float* pred = p.pred + start;
  const float* gt = p.gt + start;
  const unsigned char* mask = p.mask ? p.mask + start : nullptr;
  const bool has_mask = mask != nullptr, has_conf = conf != nullptr;
  const int nb = p.nbins;
  const float nbf = static_cast<float>(nb), lastf = static_cast<float>(nb - 1);

  // Same-address LDS atomics (a confidence map's top bin) serialise; a wave-level pre-combine of equal
  // bins was built and measured and lost more than it won, so every scored pixel adds itself.
  auto take = [&](float c, float x, float g, unsigned char m) {
#pragma clang fp contract(off)
    if (!pixel_valid(has_mask, m, g)) return;
    const float e = fabsf(x - g);
    if (!(fabsf(x) < INFINITY) || (has_conf && !(c >= 0.f && c <= 1.0f))) {
      atomicAdd(drop, 1u);
      return;
    }
    int bin;
    if (has_conf) {
      bin = min(nb - 1, static_cast<int>(c * nbf));
    } else {
      const float v = e * p.err_bin_scale;
      bin = nb - 1 - (v < lastf ? static_cast<int>(v) : nb - 1);
    }
    atomicAdd(&cnt[bin], 1u);
    atomicAdd(&sum[bin], static_cast<unsigned long long>(static_cast<long long>(fminf(e, 4096.0f) * 1048576.0f)));
  };

  const long long stride = static_cast<long long>(p.blocks_per_pair) * kThreads;
  const long long t = static_cast<long long>(blockIdx.x - b * p.blocks_per_pair) * kThreads + threadIdx.x;
  long long i = t;
  for (; i + (kBatch - 1) * stride < p.P; i += kBatch * stride) {
    float c[kBatch], x[kBatch], g[kBatch];
    unsigned char m[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      const long long j = i + k * stride;
      c[k] = has_conf ? conf[j] : 0.f;
      x[k] = pred[j];
      g[k] = gt[j];
      m[k] = has_mask ? mask[j] : 0;
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) take(c[k], x[k], g[k], m[k]);
  }
  for (; i < p.P; i += stride) take(has_conf ? conf[i] : 0.f, pred[i], gt[i], has_mask ? mask[i] : 0);
  __syncthreads();

  for (int k = threadIdx.x; k < nb; k += kThreads) {
    const unsigned int n = cnt[k];
    if (n) {
      atomicAdd(&p.count[static_cast<long long>(b) * nb + k], static_cast<unsigned long long>(n));
      atomicAdd(&p.err_q20[static_cast<long long>(b) * nb + k], sum[k]);
    }
  }
  if (threadIdx.x == 0 && *drop) atomicAdd(&p.dropped[b], static_cast<unsigned long long>(*drop));
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" int fsmi_risk_coverage(const float* conf_or_null, const float* pred, const float* gt,
                                  const unsigned char* mask_or_null, int B, int H, int W, int nbins, float err_bin_scale,
                                  long long* count, long long* err_q20, long long* dropped, void* stream) {
  FSMI_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "fsmi_risk_coverage: bad shape (%d,%d,%d)", B, H, W);
  FSMI_CHECK_ARG(nbins >= 2 && nbins <= FSMI_RISK_MAX_BINS, "fsmi_risk_coverage: nbins = %d: 2..%d", nbins,
                 FSMI_RISK_MAX_BINS);
  FSMI_CHECK_ARG(err_bin_scale > 0.f && err_bin_scale < INFINITY,
                 "fsmi_risk_coverage: err_bin_scale = %g must be finite and positive", static_cast<double>(err_bin_scale));
  FSMI_CHECK_ARG(pred && gt && count && err_q20 && dropped, "fsmi_risk_coverage: null pointer");
  const long long P = static_cast<long long>(H) * W;
  FSMI_CHECK_ARG(P <= INT_MAX, "fsmi_risk_coverage: H*W = %lld exceeds 2^31 - 1", P);
  FSMI_CHECK_ARG(aligned(conf_or_null, 4) && aligned(pred, 4) && aligned(gt, 4) && aligned(count, 8) &&
                     aligned(err_q20, 8) && aligned(dropped, 8),
                 "fsmi_risk_coverage: fp32 maps must be 4-byte, int64 outputs 8-byte aligned");
  Params p;
  p.conf = conf_or_null;
  p.pred = pred;
  p.gt = gt;
  p.mask = mask_or_null;
  p.count = reinterpret_cast<unsigned long long*>(count);
  p.err_q20 = reinterpret_cast<unsigned long long*>(err_q20);
  p.dropped = reinterpret_cast<unsigned long long*>(dropped);
  p.P = P;
  p.nbins = nbins;
  p.err_bin_scale = err_bin_scale;
  p.blocks_per_pair = static_cast<int>(std::min<long long>(std::max<long long>((P + kPixelsPerBlock - 1) / kPixelsPerBlock, 1),
                                                           std::max(kMaxBlocks / B, 1)));
  const long long nblocks = static_cast<long long>(B) * p.blocks_per_pair;       // <= max(B, kMaxBlocks)
  hipStream_t s = as_stream(stream);
  const size_t row = static_cast<size_t>(B) * nbins * sizeof(long long);
  hipError_t e = hipMemsetAsync(count, 0, row, s);
  if (e == hipSuccess) e = hipMemsetAsync(err_q20, 0, row, s);
  if (e == hipSuccess) e = hipMemsetAsync(dropped, 0, static_cast<size_t>(B) * sizeof(long long), s);
  if (e != hipSuccess) {
    set_error("fsmi_risk_coverage: hipMemsetAsync failed: %s", hipGetErrorString(e));
    return static_cast<int>(e);
  }
  const size_t lds_bytes = static_cast<size_t>(nbins) * 12 + 8;
  hipLaunchKernelGGL(risk_coverage_kernel, dim3(static_cast<unsigned>(nblocks)), dim3(kThreads), lds_bytes, s, p);
  return finish_launch("fsmi_risk_coverage");
}
