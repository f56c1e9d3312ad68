// The hot loop of the reference's spectral clustering, fused so that the affinity matrix is never stored:
//   spartan/examples/spectral_clustering.py   _row_similarity_mapper (:61-83: a Python double loop over all pairs)
//                                             sum(A, axis=1)          (:121)
//                                             _laplacian_mapper       (:85-103: diag(s) A diag(s), diagonal <- 1)
// The contract is in include/spartan_hip_spectral.h.  Three kernels:
//   affinity_degree_kernel   a workgroup of 256 threads = 64 rows of X x a range of blocks of 64 rows of Y.  The distance
//                            tile is sp_d2_tile (sp_extras_common.hpp; its L1 form for 'manhattan'): thread (ty, tx) of
//                            the 16 x 16 grid holds the 4 x 4 distances of rows 4 ty .. 4 ty + 3 and columns 4 tx ..
//                            4 tx + 3.  The 16 lanes that share a row are neighbours in a wave: the row's sum over a
//                            block is a butterfly over those lanes, no LDS and no barrier.
//   sp_partial_sum_kernel    the ranges' partial degrees, added in ascending order (sp_extras_common.hpp).
//   affinity_matrix_kernel   a workgroup per 64 x 64 tile of the output: the same tile, the measure, the two scales and
//                            the diagonal in registers, a thread's four columns in aligned 16-byte stores where the layout allows.
#include <cmath>
#include <limits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_spectral.h"

namespace {

constexpr int TB = SP_AFF_TILE;        // rows and columns of a tile
constexpr int DC = SP_D2_DC;           // features per chunk of the distance tile
constexpr int PITCH = SP_D2_PITCH;     // elements between the feature rows of a staged chunk
static_assert(TB == 64, "the thread maps below are written for 64 x 64");

__device__ __forceinline__ float exp_t(float a) { return expf(a); }
__device__ __forceinline__ double exp_t(double a) { return exp(a); }

// the measure of a pair from its distance (d2, or d1 for 'manhattan'); g = T(gamma)
template <typename T, int METRIC>
__device__ __forceinline__ T aff(T dist, T g) {
  if (METRIC == SP_AFF_RBF) return exp_t(-(g * dist));
  if (METRIC == SP_AFF_EUCLIDEAN) return sqrt_t(dist);
  return dist;
}

template <typename T, int METRIC>
__global__ __launch_bounds__(256) void affinity_degree_kernel(const T* __restrict__ X, int64_t ldx, int64_t m,
                                                              const T* __restrict__ Y, int64_t ldy, int64_t n, int64_t d,
                                                              T g, int64_t ranges, T* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) T xs[DC * PITCH];
  __shared__ __attribute__((aligned(16))) T cs[DC * PITCH];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t r0 = (int64_t)blockIdx.x * TB, rg = blockIdx.y;
  const int64_t nb = (n + TB - 1) / TB;
  const int64_t cb_b = rg * nb / ranges, cb_e = (rg + 1) * nb / ranges;

  T z[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) z[a] = (T)0;

  T acc[4][4];
  for (int64_t cb = cb_b; cb < cb_e; ++cb) {
    const int64_t c0 = cb * TB;
    sp_d2_tile<T, METRIC == SP_AFF_MANHATTAN>(X, ldx, m, r0, Y, ldy, n, c0, d, xs, cs, tid, acc);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      T s = (T)0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t c = c0 + tx * 4 + b;
        s = s + (c < n ? aff<T, METRIC>(acc[a][b], g) : (T)0);
      }
      // the 16 lanes tx = 0 .. 15 of this row: a balanced tree (addition commutes, so every lane holds the same bits)
#pragma unroll
      for (int w = 1; w < 16; w <<= 1) s = s + __shfl_xor(s, w);
      z[a] = z[a] + s;
    }
  }

  if (tx == 0) {
    T* o = out + rg * m;                // (one range: out is D itself)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t row = r0 + ty * 4 + a;
      if (row < m) o[row] = z[a];
    }
  }
}

template <typename T, int METRIC>
__global__ __launch_bounds__(256) void affinity_matrix_kernel(const T* __restrict__ X, int64_t ldx, int64_t m, int64_t r0g,
                                                              const T* __restrict__ Y, int64_t ldy, int64_t n, int64_t d,
                                                              T g, const T* __restrict__ S, int64_t ctiles,
                                                              T* __restrict__ out, int64_t ldo, int vec) {
  __shared__ __attribute__((aligned(16))) T xs[DC * PITCH];
  __shared__ __attribute__((aligned(16))) T cs[DC * PITCH];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t bid = blockIdx.x;
  const int64_t r0 = (bid / ctiles) * TB, c0 = (bid % ctiles) * TB;

  T acc[4][4];
  sp_d2_tile<T, METRIC == SP_AFF_MANHATTAN>(X, ldx, m, r0, Y, ldy, n, c0, d, xs, cs, tid, acc);

  const int64_t cl = c0 + tx * 4;
  T sc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) sc[b] = (S && cl + b < n) ? S[cl + b] : (T)1;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int64_t row = r0 + ty * 4 + a;
    if (row >= m) continue;
    const T sr = S ? S[r0g + row] : (T)1;
    Vec4<T> v;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      T e = aff<T, METRIC>(acc[a][b], g);
      if (S) {
        e = e * (sr * sc[b]);
        if (cl + b == r0g + row) e = (T)1;
      }
      v.v[b] = e;
    }
    T* o = out + row * ldo + cl;
    if (vec && cl + 3 < n) {
      *reinterpret_cast<Vec4<T>*>(o) = v;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (cl + b < n) o[b] = v.v[b];
    }
  }
}

// the number of ranges the blocks of 64 columns are cut into: from n alone
int64_t aff_ranges(int64_t n) {
  const int64_t nb = (n + TB - 1) / TB;
  int64_t r = nb / SP_AFF_RANGE_BLOCKS;
  if (r > SP_AFF_MAX_RANGES) r = SP_AFF_MAX_RANGES;
  return r < 1 ? 1 : r;
}

size_t aff_ws_bytes(size_t sz, int64_t m, int64_t n) {
  const int64_t ranges = aff_ranges(n);
  return ranges > 1 ? (size_t)ranges * (size_t)m * sz : 0;
}

// the checks both entry points share; 0 when the arguments are taken.  tmax: the largest finite T
int aff_check(const char* name, int32_t metric, double gamma, double tmax, int64_t ldx, int64_t m, int64_t ldy, int64_t n,
              int64_t d) {
  if (metric != SP_AFF_RBF && metric != SP_AFF_EUCLIDEAN && metric != SP_AFF_MANHATTAN)
    SP_FAIL("%s: unknown metric %d (0 rbf, 1 euclidean, 2 manhattan)", name, (int)metric);
  if (!(std::fabs(gamma) <= tmax)) SP_FAIL("%s: gamma = %g must be finite in the operands' dtype", name, gamma);
  if (m < 0 || n < 0 || d < 0 || ldx < d || ldy < d)
    SP_FAIL("%s: bad shape m=%lld n=%lld d=%lld ldx=%lld ldy=%lld", name, (long long)m, (long long)n, (long long)d,
            (long long)ldx, (long long)ldy);
  return 0;
}

template <typename T, int METRIC>
int degree_run(const T* X, int64_t ldx, int64_t m, const T* Y, int64_t ldy, int64_t n, int64_t d, T g, T* D, void* ws,
               hipStream_t st) {
  const int64_t ranges = aff_ranges(n), rb = (m + TB - 1) / TB;
  T* part = ranges > 1 ? reinterpret_cast<T*>(ws) : D;
  hipLaunchKernelGGL((affinity_degree_kernel<T, METRIC>), dim3((unsigned)rb, (unsigned)ranges), dim3(256), 0, st, X, ldx, m,
                     Y, ldy, n, d, g, ranges, part);
  SP_CHECK_LAUNCH();
  // D[i] <- P_0[i] + P_1[i] + ... in ascending range order
  if (ranges > 1) return sp_partial_sum<T>(part, ranges, m, 1, D, 1, nullptr, 0, nullptr, st);
  return 0;
}

template <typename T, int METRIC>
int matrix_run(const T* X, int64_t ldx, int64_t m, int64_t r0, const T* Y, int64_t ldy, int64_t n, int64_t d, T g,
               const T* S, T* out, int64_t ldo, hipStream_t st) {
  const int64_t rtiles = (m + TB - 1) / TB, ctiles = (n + TB - 1) / TB;
  // a thread's four columns as aligned 16-byte stores: every row of `out` starts on a 16-byte boundary
  const int vec = (ldo * sizeof(T)) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  hipLaunchKernelGGL((affinity_matrix_kernel<T, METRIC>), dim3((unsigned)(rtiles * ctiles)), dim3(256), 0, st, X, ldx, m,
                     r0, Y, ldy, n, d, g, S, ctiles, out, ldo, vec);
  SP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t sp_affinity_degree_workspace_bytes(int32_t dtype, int64_t m, int64_t n, int64_t d) {
  if ((dtype != SP_F32 && dtype != SP_F64) || m < 0 || n < 0 || d < 0) return 0;
  return aff_ws_bytes(sp_dtype_size(dtype), m, n);
}

extern "C" int sp_affinity_degree(int32_t dtype, int32_t metric, double gamma, const void* d_X, int64_t ldx, int64_t m,
                                  const void* d_Y, int64_t ldy, int64_t n, int64_t d, void* d_D, void* d_ws,
                                  size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_affinity_degree", dtype, [&](auto t) -> int {
    using T = decltype(t);
    const double tmax = (double)std::numeric_limits<T>::max();
    if (aff_check("sp_affinity_degree", metric, gamma, tmax, ldx, m, ldy, n, d)) return 1;
    if (m == 0) return 0;
    if (!d_D) SP_FAIL("sp_affinity_degree: D is required");
    if (d > 0 && (!d_X || (n > 0 && !d_Y))) SP_FAIL("sp_affinity_degree: X and Y are required");
    const size_t need = aff_ws_bytes(sizeof(T), m, n);
    if (need && (!d_ws || ws_bytes < need))
      SP_FAIL("sp_affinity_degree: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
    if ((m + TB - 1) / TB > 0x7fffffffLL)
      SP_FAIL("sp_affinity_degree: m=%lld is too many workgroups for one launch", (long long)m);
    const T* X = (const T*)d_X;
    const T* Y = (const T*)d_Y;
    hipStream_t st = (hipStream_t)stream;
    if (metric == SP_AFF_RBF) return degree_run<T, SP_AFF_RBF>(X, ldx, m, Y, ldy, n, d, (T)gamma, (T*)d_D, d_ws, st);
    if (metric == SP_AFF_EUCLIDEAN)
      return degree_run<T, SP_AFF_EUCLIDEAN>(X, ldx, m, Y, ldy, n, d, (T)gamma, (T*)d_D, d_ws, st);
    return degree_run<T, SP_AFF_MANHATTAN>(X, ldx, m, Y, ldy, n, d, (T)gamma, (T*)d_D, d_ws, st);
  });
}

extern "C" int sp_affinity_matrix(int32_t dtype, int32_t metric, double gamma, const void* d_X, int64_t ldx, int64_t m,
                                  int64_t r0, const void* d_Y, int64_t ldy, int64_t n, int64_t d, const void* d_S,
                                  void* d_out, int64_t ldo, void* stream) {
  return sp_float_dispatch("sp_affinity_matrix", dtype, [&](auto t) -> int {
    using T = decltype(t);
    const double tmax = (double)std::numeric_limits<T>::max();
    if (aff_check("sp_affinity_matrix", metric, gamma, tmax, ldx, m, ldy, n, d)) return 1;
    if (r0 < 0 || r0 > n - m)
      SP_FAIL("sp_affinity_matrix: rows r0=%lld .. r0+m=%lld are not among the n=%lld points", (long long)r0,
              (long long)(r0 + m), (long long)n);
    if (ldo < n) SP_FAIL("sp_affinity_matrix: bad shape n=%lld ldo=%lld", (long long)n, (long long)ldo);
    if (m == 0 || n == 0) return 0;
    if (!d_out) SP_FAIL("sp_affinity_matrix: out is required");
    if (d > 0 && (!d_X || !d_Y)) SP_FAIL("sp_affinity_matrix: X and Y are required");
    if ((double)((m + TB - 1) / TB) * (double)((n + TB - 1) / TB) > 2147483647.0)
      SP_FAIL("sp_affinity_matrix: m=%lld n=%lld are too many workgroups for one launch", (long long)m, (long long)n);
    const T* X = (const T*)d_X;
    const T* Y = (const T*)d_Y;
    const T* S = (const T*)d_S;
    hipStream_t st = (hipStream_t)stream;
    if (metric == SP_AFF_RBF)
      return matrix_run<T, SP_AFF_RBF>(X, ldx, m, r0, Y, ldy, n, d, (T)gamma, S, (T*)d_out, ldo, st);
    if (metric == SP_AFF_EUCLIDEAN)
      return matrix_run<T, SP_AFF_EUCLIDEAN>(X, ldx, m, r0, Y, ldy, n, d, (T)gamma, S, (T*)d_out, ldo, st);
    return matrix_run<T, SP_AFF_MANHATTAN>(X, ldx, m, r0, Y, ldy, n, d, (T)gamma, S, (T*)d_out, ldo, st);
  });
}
