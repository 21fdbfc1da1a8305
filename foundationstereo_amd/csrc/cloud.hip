// After the forward: disparity -> metric XYZ map (scripts/run_demo.py:173-251, Utils.py:56-75) and the
// radius outlier filter the demo applies to the cloud (scripts/run_demo.py:270-273, Open3D's
// remove_radius_outlier) as a uniform-grid neighbour count.  Three kernels:
//   disp_to_xyz   a pure stream, 4 B read + 17 B written per pixel
//   cell_keys     one int64 grid-cell key per point (sorted by torch.sort in the caller)
//   radius_count  per point, the 9 (dx,dy) cell columns around it: binary search for the column's
//                 contiguous key range, then a wave-wide distance test over the points gathered in
//                 key order
#include <climits>
#include <cstdint>

#include "fsmi_common.h"

namespace fsmi {
namespace {

struct Camera {
  float fx, fy, cx, cy, baseline, zmin, z_far;
  int remove_invisible, panorama;
};

struct Pixel {
  float x, y, z, depth;
  unsigned char valid;
};

constexpr float kPi = 3.14159265358979323846f;

// One pixel (column u, row v).  The IEEE division and the un-contracted products keep each value
// within a few fp32 roundings of the fp64 restatement (tests/cloud_oracle.py).
__device__ __forceinline__ Pixel unproject(float d, int u, int v, int H, int W, const Camera& c) {
#pragma clang fp contract(off)
  Pixel o;
  const float fu = static_cast<float>(u), fv = static_cast<float>(v);
  const float us_right = fu - d;
  // run_demo.py:174-178: disp[xx - disp < 0] = inf (false for NaN, as in numpy)
  const bool removed = c.remove_invisible && us_right < 0.f;
  float px, py, pz, dep;
  bool ok;
  if (!c.panorama) {
    // run_demo.py:235 depth = fx * b / disp; Utils.py:57,68-74 xyz, zeroed where depth < zmin
    const float z = removed ? 0.f : c.fx * c.baseline / d;
    dep = z;
    const bool keep = isfinite(z) && !(z < c.zmin);
    pz = keep ? z : 0.f;
    px = keep ? (fu - c.cx) * z / c.fx : 0.f;
    py = keep ? (fv - c.cy) * z / c.fy : 0.f;
    // run_demo.py:240,249: not removed, z > 0 (after the zmin zeroing), z <= z_far
    ok = !removed && isfinite(d) && pz > 0.f && pz <= c.z_far;
  } else {
    // run_demo.py:186-219, the up/down ERP rig; rows pair with longitude and columns with latitude,
    // as the reference writes it
    const float lon_up = (fv * 2.f / static_cast<float>(H) - 1.f) * kPi;
    const float lat_up = (fu * 2.f / static_cast<float>(W) - 1.f) * (kPi / 2.f);
    const float lat_down = (us_right * 2.f / static_cast<float>(W) - 1.f) * (kPi / 2.f);
    const float ang_disp = d * 2.f * kPi / static_cast<float>(W);
    const float tr = removed ? 0.f : c.baseline * cosf(lat_down) / sinf(ang_disp);
    dep = tr;
    const bool fin = isfinite(tr);
    const float cl = cosf(lat_up);
    px = fin ? sinf(lat_up) * tr : 0.f;
    py = fin ? -cl * cosf(lon_up) * tr : 0.f;
    pz = fin ? cl * sinf(lon_up) * tr : 0.f;
    ok = !removed && fin && tr > 0.f;
  }
  o.x = px; o.y = py; o.z = pz; o.depth = dep;
  o.valid = ok ? 1 : 0;
  return o;
}

// One thread owns 4 consecutive pixels of the flat (B,H,W) index, so every vector access is 16-B
// aligned whatever W is (a pixel of xyz is 12 B: a quad starts at 48 q bytes): one float4 load, three
// float4 stores of xyz, one float4 of depth and one 32-bit store of the 4 valid bytes.  A quad may
// run over a row end; the column / row of each of its pixels is stepped, not divided.  The last
// P % 4 pixels go through the scalar path of the thread after the last quad.
__global__ __launch_bounds__(256) void disp_to_xyz_kernel(const float* __restrict__ disp, float* __restrict__ xyz,
                                                          float* __restrict__ depth,
                                                          unsigned char* __restrict__ valid, int H, int W,
                                                          long long P, Camera cam) {
  const long long q = blockIdx.x * 256ll + threadIdx.x;
  const long long nquad = P >> 2;
  if (q > nquad) return;
  const long long p0 = q << 2;
  const long long row = p0 / W;
  int u = static_cast<int>(p0 - row * W);
  int v = static_cast<int>(row % H);
  if (q < nquad) {
    const float4 d4 = *reinterpret_cast<const float4*>(disp + p0);
    const float d[4] = {d4.x, d4.y, d4.z, d4.w};
    Pixel o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = unproject(d[k], u, v, H, W, cam);
      if (++u == W) {
        u = 0;
        if (++v == H) v = 0;
      }
    }
    float4* xo = reinterpret_cast<float4*>(xyz + 3 * p0);
    xo[0] = make_float4(o[0].x, o[0].y, o[0].z, o[1].x);
    xo[1] = make_float4(o[1].y, o[1].z, o[2].x, o[2].y);
    xo[2] = make_float4(o[2].z, o[3].x, o[3].y, o[3].z);
    *reinterpret_cast<float4*>(depth + p0) = make_float4(o[0].depth, o[1].depth, o[2].depth, o[3].depth);
    *reinterpret_cast<uchar4*>(valid + p0) = make_uchar4(o[0].valid, o[1].valid, o[2].valid, o[3].valid);
  } else {
    for (long long p = p0; p < P; ++p) {
      const Pixel o = unproject(disp[p], u, v, H, W, cam);
      xyz[3 * p] = o.x;
      xyz[3 * p + 1] = o.y;
      xyz[3 * p + 2] = o.z;
      depth[p] = o.depth;
      valid[p] = o.valid;
      if (++u == W) {
        u = 0;
        if (++v == H) v = 0;
      }
    }
  }
}

// ---- uniform grid ----------------------------------------------------------
constexpr int kCellMax = (1 << 20) - 1;          // indices clamp to +-kCellMax
constexpr int kCellTop = 2 * kCellMax;           // largest biased index (21 bits)
constexpr long long kInvalidKey = LLONG_MAX;

__host__ __device__ __forceinline__ long long pack_key(int ix, int iy, int iz) {
  return (static_cast<long long>(ix) << 42) | (static_cast<long long>(iy) << 21) | static_cast<long long>(iz);
}

// cell = radius (1 + 2^-20), so two points closer than radius differ by less than 1 - 2^-21 in
// coord / cell and sit at most one cell apart.  The quotient is taken in fp64: rounded to fp32 it
// moves the cell boundaries by half an ulp of the index, and where the index crosses a power of two
// >= 32 that narrows one cell by more than the margin.
__device__ __forceinline__ int cell_index(float coord, double inv_cell) {
  double q = floor(static_cast<double>(coord) * inv_cell);
  q = fmin(fmax(q, -static_cast<double>(kCellMax)), static_cast<double>(kCellMax));
  return static_cast<int>(q) + kCellMax;
}

__global__ __launch_bounds__(256) void cell_keys_kernel(const float* __restrict__ pts,
                                                        const unsigned char* __restrict__ valid,
                                                        long long* __restrict__ keys, int N, double inv_cell) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float x = pts[3 * static_cast<size_t>(i)], y = pts[3 * static_cast<size_t>(i) + 1],
              z = pts[3 * static_cast<size_t>(i) + 2];
  const bool ok = (!valid || valid[i]) && isfinite(x) && isfinite(y) && isfinite(z);
  keys[i] = ok ? pack_key(cell_index(x, inv_cell), cell_index(y, inv_cell), cell_index(z, inv_cell)) : kInvalidKey;
}

// first index in [0, n) whose key is >= k
__device__ __forceinline__ int lower_bound(const long long* __restrict__ keys, int n, long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void column_offset(int c, int& dx, int& dy) {
  // 0: centre; 1-4: edge neighbours; 5-8: corners
  dx = c == 0 ? 0 : c < 5 ? ((c == 1) ? -1 : (c == 2) ? 1 : 0) : ((c & 1) ? -1 : 1);
  dy = c == 0 ? 0 : c < 5 ? ((c == 3) ? -1 : (c == 4) ? 1 : 0) : ((c < 7) ? -1 : 1);
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// One wave per 64 consecutive sorted slots, in two phases.  Phase 1, a lane per point: the start of
// each of its 9 column ranges by binary search (the searches of neighbouring lanes hit the same
// lines).  Phase 2, a point at a time with the whole wave on it: the lanes take 64 consecutive
// candidates of a column (one coalesced 1-KiB read of points, 512 B of keys), a ballot counts the hits,
// and the point is left as soon as the count passes nb_points -- the exit is wave-uniform, so an
// outlier that walks all 27 cells does not hold 63 finished lanes (one thread per point did: 5.5x
// slower at 640x480).  z is the low field of the key, so the three cells (cx, cy, z-1..z+1)
// of a column are one contiguous range; the centre column goes first and the corners last.
__global__ __launch_bounds__(256) void radius_count_kernel(const long long* __restrict__ keys,
                                                           const long long* __restrict__ perm,
                                                           const float4* __restrict__ pts,
                                                           unsigned char* __restrict__ keep, int N, float r2,
                                                           int nb_points) {
  const int lane = threadIdx.x & 63;
  const int base = __builtin_amdgcn_readfirstlane(blockIdx.x * 256 + (threadIdx.x & ~63));
  if (base >= N) return;                                  // wave-uniform
  const int npts = min(64, N - base);
  const int i = min(base + lane, N - 1);                  // lanes past the end repeat the last slot, write nothing
  const long long key = keys[i];
  const float4 self = pts[i];
  const bool ok = key != kInvalidKey;
  const int ix = static_cast<int>(key >> 42), iy = static_cast<int>((key >> 21) & 0x1fffff),
            iz = static_cast<int>(key & 0x1fffff);
  int start[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    int dx, dy;
    column_offset(c, dx, dy);
    const int cx = ix + dx, cy = iy + dy;
    const bool in = ok && cx >= 0 && cx <= kCellTop && cy >= 0 && cy <= kCellTop;
    start[c] = in ? lower_bound(keys, N, pack_key(cx, cy, max(iz - 1, 0))) : N;   // N: an empty range
  }
  bool mine = false;
  for (int p = 0; p < npts; ++p) {                        // wave-uniform loop
    const int klo = __builtin_amdgcn_readlane(static_cast<int>(key), p);
    const int khi32 = __builtin_amdgcn_readlane(static_cast<int>(key >> 32), p);
    const long long kp = (static_cast<long long>(khi32) << 32) | static_cast<unsigned>(klo);
    if (kp == kInvalidKey) continue;
    const int pix = static_cast<int>(kp >> 42), piy = static_cast<int>((kp >> 21) & 0x1fffff),
              piz = static_cast<int>(kp & 0x1fffff);
    const int zhi = min(piz + 1, kCellTop);
    const float px = lane_value(self.x, p), py = lane_value(self.y, p), pz = lane_value(self.z, p);
    int count = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      int dx, dy;
      column_offset(c, dx, dy);
      const long long last = pack_key(pix + dx, piy + dy, zhi);     // unused when the range is empty
      int j0 = __builtin_amdgcn_readlane(start[c], p);
      while (j0 < N) {
        const int j = j0 + lane;
        const bool in = j < N && keys[min(j, N - 1)] <= last;
        bool hit = false;
        if (in) {
          const float4 o = pts[j];
          const float ex = o.x - px, ey = o.y - py, ez = o.z - pz;
          hit = ex * ex + ey * ey + ez * ez < r2;
        }
        count += __popcll(__builtin_amdgcn_ballot_w64(hit));
        if (count > nb_points || __builtin_amdgcn_ballot_w64(in) != ~0ull) break;   // done, or the range ended
        j0 += 64;
      }
      if (count > nb_points) break;
    }
    if (lane == p) mine = count > nb_points;
  }
  if (base + lane < N) {
    const long long dst = perm[i];
    if (dst >= 0 && dst < N) keep[dst] = mine ? 1 : 0;    // not a permutation of [0, N): nothing out of range
  }
}

}  // namespace
}  // namespace fsmi

using namespace fsmi;

extern "C" {

int fsmi_disp_to_xyz(const float* disp, float* xyz, float* depth, unsigned char* valid, int B, int H, int W,
                     float fx, float fy, float cx, float cy, float baseline, float zmin, float z_far,
                     int remove_invisible, int camera_type, void* stream) {
  FSMI_CHECK_ARG(disp && xyz && depth && valid, "fsmi_disp_to_xyz: null pointer");
  FSMI_CHECK_ARG(B > 0 && H > 0 && W > 0, "fsmi_disp_to_xyz: bad shape (%d,%d,%d)", B, H, W);
  const long long P = static_cast<long long>(B) * H * W;
  FSMI_CHECK_ARG(static_cast<long long>(H) * W <= INT_MAX && P <= INT_MAX,
                 "fsmi_disp_to_xyz: B*H*W = %lld exceeds 2^31 - 1", P);
  FSMI_CHECK_ARG(camera_type == FSMI_CAMERA_PINHOLE || camera_type == FSMI_CAMERA_PANORAMA,
                 "fsmi_disp_to_xyz: camera_type %d", camera_type);
  FSMI_CHECK_ARG(camera_type == FSMI_CAMERA_PANORAMA || (fx != 0.f && fy != 0.f && std::isfinite(fx) && std::isfinite(fy)),
                 "fsmi_disp_to_xyz: fx, fy must be finite and nonzero");
  FSMI_CHECK_ARG(aligned(disp, 16) && aligned(xyz, 16) && aligned(depth, 16) && aligned(valid, 4),
                 "fsmi_disp_to_xyz: disp, xyz, depth must be 16-byte aligned and valid 4-byte aligned");
  Camera cam{fx, fy, cx, cy, baseline, zmin, z_far, remove_invisible != 0, camera_type == FSMI_CAMERA_PANORAMA};
  const long long nthreads = (P >> 2) + ((P & 3) ? 1 : 0);
  hipLaunchKernelGGL(disp_to_xyz_kernel, dim3(ceil_div(nthreads, 256)), dim3(256), 0, as_stream(stream), disp, xyz,
                     depth, valid, H, W, P, cam);
  return finish_launch("fsmi_disp_to_xyz");
}

int fsmi_cloud_cell_keys(const float* points, const unsigned char* valid, long long* keys, int N, float radius,
                         void* stream) {
  FSMI_CHECK_ARG(N >= 0 && N <= INT_MAX - 256, "fsmi_cloud_cell_keys: N = %d", N);
  FSMI_CHECK_ARG(radius > 0.f && std::isfinite(radius), "fsmi_cloud_cell_keys: radius must be positive and finite");
  if (N == 0) return FSMI_OK;
  FSMI_CHECK_ARG(points && keys, "fsmi_cloud_cell_keys: null pointer");
  const float cell = radius * (1.0f + 0x1p-20f);
  hipLaunchKernelGGL(cell_keys_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, as_stream(stream), points, valid, keys,
                     N, 1.0 / static_cast<double>(cell));
  return finish_launch("fsmi_cloud_cell_keys");
}

int fsmi_radius_count(const long long* sorted_keys, const long long* perm, const float* sorted_points4,
                      unsigned char* keep, int N, float radius, int nb_points, void* stream) {
  FSMI_CHECK_ARG(N >= 0 && N <= INT_MAX - 256, "fsmi_radius_count: N = %d", N);   // slot + lane stays an int
  FSMI_CHECK_ARG(radius > 0.f && std::isfinite(radius), "fsmi_radius_count: radius must be positive and finite");
  FSMI_CHECK_ARG(nb_points >= 0, "fsmi_radius_count: nb_points = %d", nb_points);
  if (N == 0) return FSMI_OK;
  FSMI_CHECK_ARG(sorted_keys && perm && sorted_points4 && keep, "fsmi_radius_count: null pointer");
  FSMI_CHECK_ARG(aligned(sorted_points4, 16), "fsmi_radius_count: sorted_points4 must be 16-byte aligned");
  hipLaunchKernelGGL(radius_count_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, as_stream(stream), sorted_keys, perm,
                     reinterpret_cast<const float4*>(sorted_points4), keep, N, radius * radius, nb_points);
  return finish_launch("fsmi_radius_count");
}

}  // extern "C"
