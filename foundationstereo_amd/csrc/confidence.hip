// How sure the cost volume was of a disparity (include/fsmi.h has the contract): the classifier's
// logits (B,D,h,w) -> up to four confidence maps on the full-resolution grid, in one launch.
//   One lane per quarter-resolution column, lanes over w: every plane load is coalesced, as in
//   softmax_regression_kernel (heads.hip).  The lane computes the column's statistics once (max, s,
//   sum e t, mu, var), then walks its up x up output pixels; only `mass` needs the column again there,
//   and only the few bins under the trapezoid (L1 / L2 hits).
//   REG > 0: the column lives in REG registers (D <= REG), HBM is read once and e_d overwrites x_d, so
//   each element costs one expf.  REG == 0: the streaming path for D > 128, three passes over the
//   column, the second and third from cache.
// 64-thread workgroups: at 640x480 with one pair there are 19 200 columns for 256 CUs, so 300 one-wave
// workgroups reach every CU where 75 four-wave ones would leave 181 idle.
#include <climits>

#include "fsmi_common.h"

namespace fsmi {
namespace {

constexpr int kThreads = 64;
constexpr int kMaxReg = 128;              // the widest register-resident column

struct Params {
  const float* logits;
  const float* disp;                      // null: self mode
  float* mass;
  float* spread;
  float* peak;
  float* entropy;
  long long ncols;                        // B * h * w
  int D, h, w, up;
  int nb;                                 // bins read per query: min(ceil(2 r1) + 3, D)
  float disp_scale, r1, ln_d;             // r1 = radius + 1, ln_d = logf(D), both formed on the host
};

struct Column {
  float m, s, mu, var, peak, entropy;
  bool bad;                               // NaN / +inf logit, or nothing but -inf: every map is NaN
};

// fsmi.h's sums, in its order.  e(d) returns e_d (and t_d through its second argument) for d = 0 .. D-1.
template <class E>
__device__ __forceinline__ void accumulate(int D, E&& e, float& s, float& set, float& sd) {
#pragma clang fp contract(off)
  for (int d = 0; d < D; ++d) {
    float t;
    const float ed = e(d, t);
    s += ed;
    set += ed != 0.f ? ed * t : 0.f;
    sd += ed * static_cast<float>(d);
  }
}

__device__ __forceinline__ void finish(Column& c, float set, const Params& p) {
#pragma clang fp contract(off)
  c.peak = 1.0f / c.s;
  const float hn = logf(c.s) - set / c.s;
  c.entropy = p.D == 1 ? 1.0f : fminf(fmaxf(1.0f - hn / p.ln_d, 0.f), 1.0f);
}

template <int REG>
__device__ __forceinline__ Column column_stats(const float* __restrict__ src, size_t hw, const Params& p) {
#pragma clang fp contract(off)
  const int D = p.D;
  Column c;
  float m = -INFINITY, s = 0.f, set = 0.f, sd = 0.f, sv = 0.f;
  bool nonfinite = false;
  if constexpr (REG > 0) {
    float x[REG];                         // past D: -inf, which every sum below takes as an exact 0
#pragma unroll
    for (int d = 0; d < REG; ++d) x[d] = d < D ? src[d * hw] : -INFINITY;
#pragma unroll
    for (int d = 0; d < REG; ++d) {
      nonfinite |= !(x[d] < INFINITY);    // NaN or +inf
      m = fmaxf(m, x[d]);
    }
#pragma unroll
    for (int d = 0; d < REG; ++d) {
      const float t = x[d] - m, ed = expf(t);
      x[d] = ed;
      s += ed;
      set += ed != 0.f ? ed * t : 0.f;
      sd += ed * static_cast<float>(d);
    }
    c.mu = sd / s;
#pragma unroll
    for (int d = 0; d < REG; ++d) {
      const float dm = static_cast<float>(d) - c.mu;
      sv += x[d] * (dm * dm);
    }
  } else {
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
      const float v = src[d * hw];
      nonfinite |= !(v < INFINITY);
      m = fmaxf(m, v);
    }
    accumulate(D, [&](int d, float& t) { t = src[d * hw] - m; return expf(t); }, s, set, sd);
    c.mu = sd / s;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
      const float dm = static_cast<float>(d) - c.mu;
      sv += expf(src[d * hw] - m) * (dm * dm);
    }
  }
  c.m = m;
  c.s = s;
  c.var = sv / s;
  c.bad = nonfinite || m == -INFINITY;
  finish(c, set, p);
  return c;
}

// mass and spread of N output pixels of one column with the queries q.  The bins under a trapezoid are
// lo = floorf(q - r1) .. lo + nb - 1 with nb = ceil(2 r1) + 3 (every other bin has weight 0 and adds an
// exact 0, so each sum equals the one over d = 0 .. D-1 in order); they are re-read four bins of every
// pixel at a time, 4 N independent loads in flight where a bin-by-bin loop would wait for each (the
// loads hit L1 / L2, and their latency is all this part costs).  A bin outside [0, D-1] or past nb is
// not loaded and enters as -inf, e = 0.  lo is clipped to [-nb, D] before the conversion, which keeps
// every bin that exists and never converts an out-of-range float.
template <int N>
__device__ __forceinline__ void pixels(const float* __restrict__ src, size_t hw, const Column& c, const float (&q)[N],
                                       const Params& p, bool want_mass, float* __restrict__ mass,
                                       float* __restrict__ spread) {
#pragma clang fp contract(off)
  const float nan = __builtin_nanf("");
  bool ok[N];
  int lo[N];
  float acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ok[i] = !c.bad && fabsf(q[i]) < INFINITY;
    const float dq = c.mu - q[i];
    spread[i] = ok[i] ? sqrtf(c.var + dq * dq) : nan;
    lo[i] = p.nb == p.D ? 0 : static_cast<int>(fminf(fmaxf(floorf(q[i] - p.r1), -static_cast<float>(p.nb)),
                                                      static_cast<float>(p.D)));
    acc[i] = 0.f;
  }
  if (!want_mass) return;
  for (int k0 = 0; k0 < p.nb; k0 += 4) {
    float x[N][4];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = lo[i] + k0 + k;
        x[i][k] = (k0 + k < p.nb && d >= 0 && d < p.D) ? src[d * hw] : -INFINITY;
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float df = static_cast<float>(lo[i] + k0 + k);
        const float wd = fminf(fmaxf(p.r1 - fabsf(df - q[i]), 0.f), 1.0f);
        acc[i] += expf(x[i][k] - c.m) * wd;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) mass[i] = ok[i] ? fminf(acc[i] / c.s, 1.0f) : nan;
}

template <int UP>
__device__ __forceinline__ void store_row(float* __restrict__ dst, const float (&v)[FSMI_CONF_MAX_UP], int up) {
  if constexpr (UP == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int i = 0; i < up; ++i) dst[i] = v[i];
  }
}

// UP == 4: the model's case, 16-byte loads and stores (a row of a map starts at a multiple of 4 floats
// and so does the lane's x * 4, so 16-byte aligned bases make every access aligned); UP == 0: any up in
// 1..8 and any 4-byte aligned base, one float at a time.
template <int REG, int UP>
__global__ __launch_bounds__(kThreads) void disp_confidence_kernel(Params p) {
  const long long col = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
  if (col >= p.ncols) return;
  const size_t hw = static_cast<size_t>(p.h) * p.w;
  const long long b = col / static_cast<long long>(hw);
  const int r = static_cast<int>(col - b * static_cast<long long>(hw));
  const int yl = r / p.w, xl = r - yl * p.w;
  const float* src = p.logits + static_cast<size_t>(b) * p.D * hw + r;
  const Column c = column_stats<REG>(src, hw, p);

  const int up = UP == 4 ? 4 : p.up;
  const size_t W = static_cast<size_t>(p.w) * up, H = static_cast<size_t>(p.h) * up;
  const float nan = __builtin_nanf("");
  const float pk = c.bad ? nan : c.peak, en = c.bad ? nan : c.entropy;
  const bool want_mass = p.mass != nullptr, want_q = want_mass || p.spread != nullptr;
  float ms[FSMI_CONF_MAX_UP], sp[FSMI_CONF_MAX_UP], pks[FSMI_CONF_MAX_UP], ens[FSMI_CONF_MAX_UP];
#pragma unroll
  for (int i = 0; i < FSMI_CONF_MAX_UP; ++i) { pks[i] = pk; ens[i] = en; ms[i] = sp[i] = nan; }
  if (want_q && !p.disp) {                  // self mode: one query for the whole column
    const float q1[1] = {c.mu};
    float m1[1], s1[1];
    pixels<1>(src, hw, c, q1, p, want_mass, m1, s1);
#pragma unroll
    for (int i = 0; i < FSMI_CONF_MAX_UP; ++i) { ms[i] = m1[0]; sp[i] = s1[0]; }
  }
  for (int dy = 0; dy < up; ++dy) {
    const size_t o = (static_cast<size_t>(b) * H + static_cast<size_t>(yl) * up + dy) * W + static_cast<size_t>(xl) * up;
    if (want_q && p.disp) {
#pragma clang fp contract(off)
      if constexpr (UP == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p.disp + o);
        const float q[4] = {v.x * p.disp_scale, v.y * p.disp_scale, v.z * p.disp_scale, v.w * p.disp_scale};
        pixels<4>(src, hw, c, q, p, want_mass, ms, sp);
      } else {
        for (int i = 0; i < up; ++i) {
          const float q[1] = {p.disp[o + i] * p.disp_scale};
          pixels<1>(src, hw, c, q, p, want_mass, ms + i, sp + i);
        }
      }
    }
    if (p.mass) store_row<UP>(p.mass + o, ms, up);
    if (p.spread) store_row<UP>(p.spread + o, sp, up);
    if (p.peak) store_row<UP>(p.peak + o, pks, up);
    if (p.entropy) store_row<UP>(p.entropy + o, ens, up);
  }
}

// wide: up == 4 and disp and the maps all 16-byte aligned; any other call takes the scalar kernel
template <int REG>
void launch(const Params& p, bool wide, unsigned blocks, hipStream_t s) {
  if (wide)
    hipLaunchKernelGGL((disp_confidence_kernel<REG, 4>), dim3(blocks), dim3(kThreads), 0, s, p);
  else
    hipLaunchKernelGGL((disp_confidence_kernel<REG, 0>), dim3(blocks), dim3(kThreads), 0, s, p);
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" int fsmi_disp_confidence(const float* logits, int B, int D, int h, int w, const float* disp_or_null, int up,
                                    float disp_scale, float radius, float* mass, float* spread, float* peak,
                                    float* entropy, void* stream) {
  FSMI_CHECK_ARG(B >= 1 && h >= 1 && w >= 1, "fsmi_disp_confidence: bad shape (%d,%d,%d,%d)", B, D, h, w);
  FSMI_CHECK_ARG(D >= 1 && D <= FSMI_CONF_MAX_D, "fsmi_disp_confidence: D = %d: 1..%d", D, FSMI_CONF_MAX_D);
  FSMI_CHECK_ARG(up >= 1 && up <= FSMI_CONF_MAX_UP, "fsmi_disp_confidence: up = %d: 1..%d", up, FSMI_CONF_MAX_UP);
  FSMI_CHECK_ARG(radius >= 0.f && radius < INFINITY, "fsmi_disp_confidence: radius = %g must be finite and >= 0",
                 static_cast<double>(radius));
  FSMI_CHECK_ARG(mass || spread || peak || entropy, "fsmi_disp_confidence: all four outputs are null");
  FSMI_CHECK_ARG(logits, "fsmi_disp_confidence: null logits");
  const long long P = static_cast<long long>(h) * up * w * up;
  FSMI_CHECK_ARG(P <= INT_MAX, "fsmi_disp_confidence: H*W = %lld exceeds 2^31 - 1", P);
  FSMI_CHECK_ARG(aligned(logits, 4) && aligned(disp_or_null, 4) && aligned(mass, 4) && aligned(spread, 4) &&
                     aligned(peak, 4) && aligned(entropy, 4),
                 "fsmi_disp_confidence: every pointer must be 4-byte aligned");
  const bool wide = up == 4 && aligned(disp_or_null, 16) && aligned(mass, 16) && aligned(spread, 16) &&
                    aligned(peak, 16) && aligned(entropy, 16);
  Params p;
  p.logits = logits;
  p.disp = disp_or_null;
  p.mass = mass;
  p.spread = spread;
  p.peak = peak;
  p.entropy = entropy;
  p.ncols = static_cast<long long>(B) * h * w;
  p.D = D; p.h = h; p.w = w; p.up = up;
  p.disp_scale = disp_scale;
  p.r1 = radius + 1.0f;
  p.ln_d = logf(static_cast<float>(D));
  p.nb = static_cast<int>(std::min(std::ceil(2.0 * static_cast<double>(p.r1)) + 3.0, static_cast<double>(D)));
  const long long blocks = (p.ncols + kThreads - 1) / kThreads;
  FSMI_CHECK_ARG(blocks <= INT_MAX, "fsmi_disp_confidence: %lld columns are too many", p.ncols);
  hipStream_t s = as_stream(stream);
  static_assert(kMaxReg == 128, "the tiers below end at kMaxReg");
  if (D <= 16) launch<16>(p, wide, static_cast<unsigned>(blocks), s);
  else if (D <= 64) launch<64>(p, wide, static_cast<unsigned>(blocks), s);
  else if (D <= kMaxReg) launch<128>(p, wide, static_cast<unsigned>(blocks), s);
  else launch<0>(p, wide, static_cast<unsigned>(blocks), s);
  return finish_launch("fsmi_disp_confidence");
}
