// What the kernels of libspartan_hip_extras.so share (linalg, knn, apsp, als, fuzzy, lda, spectral; the main library's
// sources do not include this file).  Every piece carries a numerical contract -- the order of an accumulation, the
// order in which partials are added -- that tests pin bit for bit: one copy, so that a fix reaches every caller.  Look
// here before copying a piece out of a neighbouring kernel file.
#pragma once
#include "sp_common.hpp"

namespace {

// N elements read or written as one aligned vector (16 bytes at the most: fp32 x 8 and fp64 x 4 are 16-byte aligned too)
template <typename T, int N>
struct alignas((sizeof(T) * N > 16 ? 16 : sizeof(T) * N)) VecN {
  T v[N];
};
template <typename T>
using Vec4 = VecN<T, 4>;

// the LDS writes of this wave above are visible to its reads below
__device__ __forceinline__ void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float sqrt_t(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_t(double a) { return __builtin_sqrt(a); }
__device__ __forceinline__ float abs_t(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double abs_t(double a) { return __builtin_fabs(a); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float pow_t(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double pow_t(double a, double b) { return pow(a, b); }

// the parts of a workspace start 256 bytes apart at the least
inline size_t sp_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the 64 x 64 squared-distance tile of sp_fuzzy_step, sp_knn and sp_affinity_* ------------------------------
constexpr int SP_D2_DC = 16;        // features per chunk
constexpr int SP_D2_PITCH = 68;     // elements between the feature rows of a staged chunk (64 + 4: 16-byte aligned rows)

// acc[a][b] <- d2 of row r0 + 4 ty + a of X and row c0 + 4 tx + b of C, thread (ty, tx) = (tid >> 4, tid & 15) of a
// workgroup of 256.  Both operands pass through LDS (xs, cs: [SP_D2_DC][SP_D2_PITCH] each) in chunks of 16 features
// stored feature-major; staging is thread (lr0 + 16 i, lj), i = 0 .. 3, of the [64 rows][16 features] chunk, so that a
// row's 16 features are one 64- or 128-byte run for 16 consecutive lanes, and the next chunk is in flight in registers
// while this one is used.  Every d2 is ONE accumulator that starts at 0 and takes (x_j - c_j)^2 for j = 0, 1, ... in
// turn.  Rows >= n of X, rows >= k of C and features >= d load 0.  Every thread of the workgroup calls it (it
// synchronises the workgroup).  knn_scan_kernel has these lines written out in its own loop and says why: a change here
// belongs there as well.  L1 (sp_affinity_*'s 'manhattan'): the term is |x_j - c_j| instead, everything else the same;
// the default leaves the squared-distance instantiations as they were.
template <typename T, bool L1 = false>
__device__ __forceinline__ void sp_d2_tile(const T* __restrict__ X, int64_t ldx, int64_t n, int64_t r0,
                                           const T* __restrict__ C, int64_t ldc, int64_t k, int64_t c0, int64_t d, T* xs,
                                           T* cs, int tid, T (&acc)[4][4]) {
  constexpr int DC = SP_D2_DC, PITCH = SP_D2_PITCH;
  const int ty = tid >> 4, tx = tid & 15;
  const int lj = tid & 15, lr0 = tid >> 4;
  const int64_t nchunks = (d + DC - 1) / DC;
  T xn[4], cn[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (T)0;

  auto fetch = [&](int64_t c) {
    const int64_t col = c * DC + lj;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t xr = r0 + lr0 + 16 * i, cr = c0 + lr0 + 16 * i;
      xn[i] = (col < d && xr < n) ? X[xr * ldx + col] : (T)0;
      cn[i] = (col < d && cr < k) ? C[cr * ldc + col] : (T)0;
    }
  };
  if (nchunks > 0) fetch(0);
  for (int64_t c = 0; c < nchunks; ++c) {
    __syncthreads();                    // the previous chunk has been read by everyone
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xs[lj * PITCH + lr0 + 16 * i] = xn[i];
      cs[lj * PITCH + lr0 + 16 * i] = cn[i];
    }
    __syncthreads();
    if (c + 1 < nchunks) fetch(c + 1);
    const int jn = (int)((d - c * DC) < DC ? (d - c * DC) : DC);
    if (jn == DC) {
#pragma unroll 4
      for (int j = 0; j < DC; ++j) {
        const Vec4<T> xv = *reinterpret_cast<const Vec4<T>*>(xs + j * PITCH + ty * 4);
        const Vec4<T> cv = *reinterpret_cast<const Vec4<T>*>(cs + j * PITCH + tx * 4);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const T t = xv.v[a] - cv.v[b];
            acc[a][b] = acc[a][b] + (L1 ? abs_t(t) : t * t);
          }
      }
    } else {
      for (int j = 0; j < jn; ++j) {
        const Vec4<T> xv = *reinterpret_cast<const Vec4<T>*>(xs + j * PITCH + ty * 4);
        const Vec4<T> cv = *reinterpret_cast<const Vec4<T>*>(cs + j * PITCH + tx * 4);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const T t = xv.v[a] - cv.v[b];
            acc[a][b] = acc[a][b] + (L1 ? abs_t(t) : t * t);
          }
      }
    }
  }
}

// ---- the sum of the ranges' partials ---------------------------------------------------------------------------------
// out[r * ldo + c] <- P_0[r, c] + P_1[r, c] + ... in ascending range order, starting from P_0 and not from 0; 0 with no
// range at all.  P_g is the contiguous rows x cols matrix at P + g * rows * cols.  The n2 elements out2[j] <- P2_0[j] +
// P2_1[j] + ... (P2_g at P2 + g * n2) are summed the same way in the same launch; n2 = 0 without a second pair.
template <typename T>
__global__ __launch_bounds__(256) void sp_partial_sum_kernel(const T* __restrict__ P, int64_t ranges, int64_t rows,
                                                             int64_t cols, T* __restrict__ out, int64_t ldo,
                                                             const T* __restrict__ P2, int64_t n2, T* __restrict__ out2) {
  const int64_t n1 = rows * cols, total = n1 + n2;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const bool first = idx < n1;
    const int64_t e = first ? idx : idx - n1, stride = first ? n1 : n2;
    const T* p = first ? P : P2;
    T a = (T)0;
    if (ranges > 0) {
      a = p[e];
      // eight loads at a time, then their additions in the same ascending order: with one load per trip the loop is
      // a chain of memory latencies, which a caller with hundreds of ranges (sp_nb_step) waits for
      int64_t g = 1;
      for (; g + 8 <= ranges; g += 8) {
        T v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[(g + i) * stride + e];
#pragma unroll
        for (int i = 0; i < 8; ++i) a = a + v[i];
      }
      for (; g < ranges; ++g) a = a + p[g * stride + e];
    }
    if (first) out[(e / cols) * ldo + e % cols] = a;
    else out2[e] = a;
  }
}

// one launch on `st`: the grid is capped at SP_CUS * SP_BLOCKS_PER_CU workgroups and strides over the rest
template <typename T>
int sp_partial_sum(const T* P, int64_t ranges, int64_t rows, int64_t cols, T* out, int64_t ldo, const T* P2, int64_t n2,
                   T* out2, hipStream_t st) {
  int64_t blocks = (rows * cols + n2 + 255) / 256;
  if (blocks > SP_CUS * SP_BLOCKS_PER_CU) blocks = SP_CUS * SP_BLOCKS_PER_CU;
  hipLaunchKernelGGL(sp_partial_sum_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, P, ranges, rows, cols, out, ldo,
                     P2, n2, out2);
  SP_CHECK_LAUNCH();
  return 0;
}

// ---- float / double entry points -------------------------------------------------------------------------------------
// run(T()) with T = float or double as `dtype` says; any other dtype is the entry point's first refusal
template <typename F>
int sp_float_dispatch(const char* name, int32_t dtype, F run) {
  if (dtype == SP_F32) return run(float());
  if (dtype == SP_F64) return run(double());
  SP_FAIL("%s: dtype must be f32 or f64; convert with astype first", name);
}

}  // namespace
