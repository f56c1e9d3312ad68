// The n x n expressions of the reference's n-body step as one all-pairs kernel:
//   spartan/examples/nbody.py   move (:71-111: dx, dy, dz, r, the mask, fx, fy, fz and their sums over axis 0)
// The contract -- the arithmetic of a pair and the order of a target's sum -- is in include/spartan_hip_nbody.h.
//   nbody_accel_kernel     a workgroup = 64 targets x a range of source blocks; lane l of each of the 4 waves holds
//                          target l, wave c the sources c, c + 4, ... of every staged block (a broadcast LDS read), the
//                          four partials per target combined through LDS as (p0 + p1) + (p2 + p3).
//   sp_partial_sum_kernel  the ranges' partial sums, added in ascending order (sp_extras_common.hpp).
#include <cmath>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_nbody.h"

namespace {

constexpr int B = SP_NBODY_BLOCK;      // sources of a block = targets of a workgroup
constexpr int W = SP_NBODY_WAVES;      // waves of a workgroup = classes the sources of a block are dealt into
static_assert(B == 64 && W == 4, "a target per lane of a wave, the staging a thread per (array, source)");

// the 16 sources k = wave, wave + 4, ... of the staged block `buf` ([64][4]: x, y, z, g * mass) onto the target's three
// accumulators, in ascending order.  CHECKED: source s0 + k adds +0 where it is the target itself or padding.
template <typename T, bool CHECKED>
__device__ __forceinline__ void nbody_block(const T* buf, int wave, int64_t s0, int64_t n, int64_t j, T xj, T yj, T zj,
                                            T rmin, T& ax, T& ay, T& az) {
#pragma unroll 4
  for (int k = wave; k < B; k += W) {
    const Vec4<T> s = *reinterpret_cast<const Vec4<T>*>(buf + k * 4);
    const T dx = s.v[0] - xj, dy = s.v[1] - yj, dz = s.v[2] - zj;
    const T q = (dx * dx + dy * dy) + dz * dz;
    T r = sqrt_t(q);
    r = r < rmin ? rmin : r;
    const T w = s.v[3] / ((r * r) * r);
    T tx = w * dx, ty = w * dy, tz = w * dz;
    if (CHECKED) {
      const int64_t i = s0 + k;
      const bool none = i == j || i >= n;
      tx = none ? (T)0 : tx;
      ty = none ? (T)0 : ty;
      tz = none ? (T)0 : tz;
    }
    ax = ax + tx;
    ay = ay + ty;
    az = az + tz;
  }
}

// workgroup blockIdx.x = (range rg) * tblocks + (target block tb).  Range rg's result for target r0 + jl goes to
// o?[rg * range_stride + jl].
template <typename T>
__global__ __launch_bounds__(256) void nbody_accel_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                                          const T* __restrict__ z, const T* __restrict__ mass, int64_t n,
                                                          T g, T rmin, int64_t r0, int64_t m, int64_t tblocks,
                                                          int64_t ranges, T* __restrict__ ox, T* __restrict__ oy,
                                                          T* __restrict__ oz, int64_t range_stride) {
  __shared__ __attribute__((aligned(16))) T src[2][B * 4];
  __shared__ T red[W][3][B];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t tb = (int64_t)blockIdx.x % tblocks, rg = (int64_t)blockIdx.x / tblocks;
  const int64_t jl = tb * B + lane;
  const bool mine = jl < m;
  const int64_t j = r0 + (mine ? jl : m - 1);       // (a lane without a target repeats the last one and stores nothing)
  const T xj = x[j], yj = y[j], zj = z[j];
  const int64_t t_lo = r0 + tb * B, t_hi = (t_lo + B < r0 + m) ? t_lo + B : r0 + m;

  const int64_t nb = (n + B - 1) / B;
  const int64_t b0 = rg * nb / ranges, b1 = (rg + 1) * nb / ranges;
  // staging: thread (wave, lane) brings element `lane` of array `wave` of a block
  const T* arr = wave == 0 ? x : wave == 1 ? y : wave == 2 ? z : mass;
  auto fetch = [&](int64_t b) {
    const int64_t i = b * B + lane;
    return i < n ? arr[i] : (T)0;
  };
  T next = b0 < b1 ? fetch(b0) : (T)0;
  T ax = (T)0, ay = (T)0, az = (T)0;
  for (int64_t b = b0; b < b1; ++b) {
    // two buffers, one barrier per block: whoever writes buffer (b - b0) & 1 again has passed the barrier of block
    // b - 1, which every wave reaches only after it has read block b - 2
    T* buf = src[(b - b0) & 1];
    buf[lane * 4 + wave] = wave == 3 ? g * next : next;
    __syncthreads();
    if (b + 1 < b1) next = fetch(b + 1);
    const int64_t s0 = b * B;
    if (s0 + B > n || (s0 < t_hi && t_lo < s0 + B))       // (the same for the whole workgroup)
      nbody_block<T, true>(buf, wave, s0, n, j, xj, yj, zj, rmin, ax, ay, az);
    else
      nbody_block<T, false>(buf, wave, s0, n, j, xj, yj, zj, rmin, ax, ay, az);
  }
  red[wave][0][lane] = ax;
  red[wave][1][lane] = ay;
  red[wave][2][lane] = az;
  __syncthreads();
  if (wave < 3 && mine) {
    const T v = (red[0][wave][lane] + red[1][wave][lane]) + (red[2][wave][lane] + red[3][wave][lane]);
    T* o = wave == 0 ? ox : wave == 1 ? oy : oz;
    o[rg * range_stride + jl] = v;
  }
}

// the number of ranges the source blocks are cut into: from n and splits alone
int64_t nbody_ranges(int64_t n, int32_t splits) {
  const int64_t nb = (n + B - 1) / B;
  if (nb <= 1) return 1;
  if (splits >= 1) return splits < nb ? splits : nb;
  const int64_t want = (SP_NBODY_WORKGROUPS + nb - 1) / nb;
  return want < nb ? want : nb;
}

size_t nbody_ws_bytes(size_t sz, int64_t n, int64_t m, int32_t splits) {
  const int64_t ranges = nbody_ranges(n, splits);
  return (ranges > 1 && m > 0) ? (size_t)ranges * 3 * (size_t)m * sz : 0;
}

template <typename T>
int nbody_run(T g, T rmin, const T* x, const T* y, const T* z, const T* mass, int64_t n, int64_t r0, int64_t m, T* ax,
              T* ay, T* az, int32_t splits, void* ws, size_t ws_bytes, hipStream_t st) {
  const int64_t ranges = nbody_ranges(n, splits), tblocks = (m + B - 1) / B;
  const size_t need = nbody_ws_bytes(sizeof(T), n, m, splits);
  if (need && (!ws || ws_bytes < need)) SP_FAIL("sp_nbody_accel: workspace of %zu bytes, %zu needed", ws_bytes, need);
  if ((double)tblocks * (double)ranges > 2147483647.0)
    SP_FAIL("sp_nbody_accel: n=%lld m=%lld are too many workgroups for one launch", (long long)n, (long long)m);
  if (m == 0) return 0;
  const unsigned grid = (unsigned)(tblocks * ranges);
  if (ranges == 1) {
    hipLaunchKernelGGL(nbody_accel_kernel<T>, dim3(grid), dim3(256), 0, st, x, y, z, mass, n, g, rmin, r0, m, tblocks,
                       ranges, ax, ay, az, (int64_t)0);
    SP_CHECK_LAUNCH();
    return 0;
  }
  T* p = reinterpret_cast<T*>(ws);
  // the three targets as the rows of one array (equal steps of at least m elements): the partials as [ranges][3][m] and
  // one sum over all of it; otherwise as [3][ranges][m], a_x and a_y summed by one launch and a_z by another
  const uintptr_t ux = (uintptr_t)ax, uy = (uintptr_t)ay, uz = (uintptr_t)az;
  const bool rows = uy > ux && uz > uy && uy - ux == uz - uy && (uy - ux) % sizeof(T) == 0 &&
                    (uy - ux) / sizeof(T) >= (uintptr_t)m;
  if (rows) {
    hipLaunchKernelGGL(nbody_accel_kernel<T>, dim3(grid), dim3(256), 0, st, x, y, z, mass, n, g, rmin, r0, m, tblocks,
                       ranges, p, p + m, p + 2 * m, 3 * m);
    SP_CHECK_LAUNCH();
    return sp_partial_sum<T>(p, ranges, 3, m, ax, (int64_t)((uy - ux) / sizeof(T)), (const T*)nullptr, 0, (T*)nullptr, st);
  }
  hipLaunchKernelGGL(nbody_accel_kernel<T>, dim3(grid), dim3(256), 0, st, x, y, z, mass, n, g, rmin, r0, m, tblocks,
                     ranges, p, p + ranges * m, p + 2 * ranges * m, m);
  SP_CHECK_LAUNCH();
  if (sp_partial_sum<T>(p, ranges, 1, m, ax, m, p + ranges * m, m, ay, st)) return 1;
  return sp_partial_sum<T>(p + 2 * ranges * m, ranges, 1, m, az, m, (const T*)nullptr, 0, (T*)nullptr, st);
}

}  // namespace

extern "C" size_t sp_nbody_accel_workspace_bytes(int32_t dtype, int64_t n, int64_t m, int32_t splits) {
  if ((dtype != SP_F32 && dtype != SP_F64) || n < 0 || m < 0 || m > n || splits < 0) return 0;
  return nbody_ws_bytes(sp_dtype_size(dtype), n, m, splits);
}

extern "C" int sp_nbody_accel(int32_t dtype, double g, double rmin, const void* d_x, const void* d_y, const void* d_z,
                              const void* d_mass, int64_t n, int64_t r0, int64_t m, void* d_ax, void* d_ay, void* d_az,
                              int32_t splits, void* d_ws, size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_nbody_accel", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0 || m < 0 || splits < 0)
      SP_FAIL("sp_nbody_accel: bad shape n=%lld m=%lld splits=%d", (long long)n, (long long)m, (int)splits);
    if (r0 < 0 || r0 > n || m > n - r0)
      SP_FAIL("sp_nbody_accel: bodies %lld .. %lld are not among the %lld", (long long)r0, (long long)(r0 + m),
              (long long)n);
    const T gt = (T)g, rt = (T)rmin;
    if (!std::isfinite(gt)) SP_FAIL("sp_nbody_accel: g = %g must be finite in the arrays' dtype", g);
    if (!(rt > (T)0) || !std::isfinite(rt))
      SP_FAIL("sp_nbody_accel: rmin = %g must be finite and > 0 in the arrays' dtype", rmin);
    if (n > 0 && (!d_x || !d_y || !d_z || !d_mass)) SP_FAIL("sp_nbody_accel: x, y, z and mass are required");
    if (m > 0 && (!d_ax || !d_ay || !d_az)) SP_FAIL("sp_nbody_accel: ax, ay and az are required");
    return nbody_run<T>(gt, rt, (const T*)d_x, (const T*)d_y, (const T*)d_z, (const T*)d_mass, n, r0, m, (T*)d_ax,
                        (T*)d_ay, (T*)d_az, splits, d_ws, ws_bytes, (hipStream_t)stream);
  });
}
