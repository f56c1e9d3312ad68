// Cholesky factorisation and triangular solve of a dense tile: the LAPACK calls inside the reference's tile bodies
//   spartan/examples/cholesky.py    _cholesky_dpotrf_mapper (:9-13)  linalg.lapack.dpotrf(tile, lower=1)
//                                   _cholesky_dtrsm_mapper (:16-20)  linalg.lapack.dtrtrs(A_kk, tile.T, lower=1).T
//   spartan/examples/ssvd/qr.py     (:37-43) np.linalg.cholesky(Y'Y) and Q = Y . inv(R), here a solve
//
// sp_potrf is blocked on two levels and LEFT-looking on both, so the matrix to the right of the block column at
// work is never touched:
//   outer block column, OB = 256 wide : takes its whole update from everything to its left in ONE long-K call of
//                                       the library's GEMM, C += A[j0:n, 0:j0] . W with W = -(A[j0:j0+w, 0:j0])^T
//                                       written into the workspace by negt_kernel (sp_gemm_* has no transposed or
//                                       negated operand);
//   inner block column, NB = 64 wide  : the same against the columns of its own outer block (K <= 192), then
//                                       potrf_block_kernel: the NB x NB diagonal block factored in LDS by one
//                                       workgroup,
//                                       trsm_rlt_kernel:    the rows below it, X . L^T = B by substitution.
// A right-looking sweep would read and write the trailing matrix once per panel; this reads the factored part once
// per OUTER block column: n^3 / (3 * OB) elements.
//
// A pivot that is not positive stops the factorisation: the block kernel writes the 1-based order of the leading
// minor to *d_info (one lane, an ordinary store) and leaves its block as it was; every later kernel of the call
// reads *d_info first and returns (negt_kernel writes zeros, so the GEMM calls, which cannot read the flag, add
// nothing).  No kernel of a failed call takes the square root of a non-positive number or divides by one.
// Square roots and divisions are the correctly rounded ones (Makefile: linalg.o).
#include "sp_common.hpp"
#include "../../include/spartan_hip_extras.h"

namespace {

constexpr int NB = 64;     // order of the block factored / solved against in LDS
constexpr int OB = 256;    // width of an outer block column (a multiple of NB)
constexpr int RB = 128;    // rows of B one workgroup of the solve owns (one per thread)
constexpr int LD = NB + 1; // LDS row stride of the block being factored: column reads hit different banks

__device__ __forceinline__ float sp_sqrt_rn(float x) { return sqrtf(x); }
__device__ __forceinline__ double sp_sqrt_rn(double x) { return sqrt(x); }

// The diagonal block A[0:bw, 0:bw] (bw <= NB, lower triangle read, lower triangle written) factored in LDS;
// `first` is the block's position in the whole matrix.  256 threads, one workgroup.
template <typename T>
__global__ __launch_bounds__(256) void potrf_block_kernel(T* __restrict__ A, int64_t lda, int bw, int64_t first,
                                                          int32_t* __restrict__ info) {
  __shared__ T S[NB * LD];
  if (*(volatile int32_t*)info != 0) return;
  const int tid = threadIdx.x;
  for (int e = tid; e < bw * bw; e += 256) {
    const int i = e / bw, j = e % bw;
    if (j <= i) S[i * LD + j] = A[(int64_t)i * lda + j];
  }
  __syncthreads();
  const int tj = tid & (NB - 1), ti = tid >> 6;     // trailing update: column tj, rows ti, ti + 4, ...
  int fail = -1;
  for (int k = 0; k < bw; ++k) {
    const T d = S[k * LD + k];                      // (every thread reads the same value: the branch is uniform)
    if (!(d > (T)0)) {
      fail = k;
      break;
    }
    const T r = sp_sqrt_rn(d);
    if (tid > k && tid < bw) S[tid * LD + k] = S[tid * LD + k] / r;
    __syncthreads();
    if (tid == 0) S[k * LD + k] = r;                // (nobody reads S[k][k] between these two barriers)
    if (tj > k && tj < bw) {
      const T ljk = S[tj * LD + k];
      for (int i = ti; i < bw; i += 4)
        if (i >= tj) S[i * LD + tj] -= S[i * LD + k] * ljk;
    }
    __syncthreads();
  }
  if (fail >= 0) {
    if (tid == 0) *info = (int32_t)(first + fail + 1);
    return;
  }
  for (int e = tid; e < bw * bw; e += 256) {
    const int i = e / bw, j = e % bw;
    if (j <= i) A[(int64_t)i * lda + j] = S[i * LD + j];
  }
}

// out[k, c] = -src[c, k] for c < N, k < K (out: K rows of ldo elements); zeros once the factorisation has failed.
// 32 x 32 tiles through LDS, block (32, 8).
template <typename T>
__global__ __launch_bounds__(256) void negt_kernel(const T* __restrict__ src, int64_t lds_, int N, int64_t K,
                                                   T* __restrict__ out, int64_t ldo, const int32_t* __restrict__ info) {
  __shared__ T t[32][33];
  const bool failed = *(volatile const int32_t*)info != 0;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int64_t k0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
#pragma unroll
  for (int s = 0; s < 32; s += 8) {
    const int c = c0 + ty + s;
    const int64_t k = k0 + tx;
    t[ty + s][tx] = (!failed && c < N && k < K) ? src[(int64_t)c * lds_ + k] : (T)0;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 32; s += 8) {
    const int64_t k = k0 + ty + s;
    const int c = c0 + tx;
    if (k < K && c < N) out[k * ldo + c] = failed ? (T)0 : -t[tx][ty + s];
  }
}

// A[i, j] = 0 for j > i: one workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void zero_upper_kernel(T* __restrict__ A, int64_t lda, int64_t n) {
  const int64_t i = blockIdx.x;
  for (int64_t j = i + 1 + threadIdx.x; j < n; j += 256) A[i * lda + j] = (T)0;
}

// B <- X with X . L^T = B; L n x n lower (its upper triangle is not read), B m x n.  A workgroup owns RB rows of B,
// one per thread, and never looks at another's: block column jb of X is
//   X_jb = (B_jb - sum_{ib < jb} X_ib . L[jb, ib]^T) . L[jb, jb]^-T
// with the NB values of the thread's row in registers, the blocks of L (transposed: Lt[k][c] = L[c][k], so that the
// c-loop reads consecutive LDS words, the same for every lane) in LDS, and X_ib read back from B, where this thread
// wrote it.  A ragged last block is padded with the identity.
template <typename T>
__global__ __launch_bounds__(RB) void trsm_rlt_kernel(const T* __restrict__ L, int64_t ldl, int64_t n, T* B, int64_t ldb,
                                                      int64_t m, const int32_t* __restrict__ info) {
  __shared__ T Lt[NB * NB + NB];
  if (threadIdx.x < NB) Lt[NB * NB + threadIdx.x] = (T)0;
  if (info != nullptr && *(volatile const int32_t*)info != 0) return;
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * RB + tid;
  const bool live = r < m;
  T* row = B + (live ? r : 0) * ldb;
  const int64_t nblk = (n + NB - 1) / NB;
  for (int64_t jb = 0; jb < nblk; ++jb) {
    const int64_t j0 = jb * NB;
    const int bw = (int)((n - j0) < NB ? (n - j0) : NB);
    T acc[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) acc[c] = (live && c < bw) ? row[j0 + c] : (T)0;
    for (int64_t ib = 0; ib < jb; ++ib) {
      __syncthreads();
      for (int e = tid; e < NB * NB; e += RB) {
        const int c = e / NB, k = e % NB;
        Lt[k * NB + c] = c < bw ? L[(j0 + c) * ldl + ib * NB + k] : (T)0;
      }
      __syncthreads();
#pragma unroll 2
      for (int k = 0; k < NB; ++k) {
        const T xk = live ? row[ib * NB + k] : (T)0;
#pragma unroll
        for (int c = 0; c < NB; ++c) acc[c] -= xk * Lt[k * NB + c];
      }
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += RB) {
      const int c = e / NB, k = e % NB;
      T v = c == k ? (T)1 : (T)0;
      if (c < bw && k < bw) v = k <= c ? L[(j0 + c) * ldl + j0 + k] : (T)0;
      Lt[k * NB + c] = v;
    }
    __syncthreads();
    // column k of the row is final once the columns before it have been taken out of it: x = acc[0] / L[k][k],
    // then the remaining columns give up x . L[c][k] and move one register down (static register numbers, a
    // rolled k-loop).  Registers past the block's end read on into the next row of Lt (the zeroed tail after the
    // last) and hold values that never move into a live register.
#pragma unroll 1
    for (int k = 0; k < bw; ++k) {
      const T* lk = Lt + k * NB + k;
      const T x = acc[0] / lk[0];
      if (live) row[j0 + k] = x;
#pragma unroll
      for (int c = 1; c < NB; ++c) acc[c - 1] = acc[c] - x * lk[c];
      acc[NB - 1] = (T)0;
    }
  }
}

template <typename T>
int trsm_launch(const T* L, int64_t ldl, int64_t n, T* B, int64_t ldb, int64_t m, const int32_t* info, hipStream_t st) {
  if (n == 0 || m == 0) return 0;
  const int64_t blocks = (m + RB - 1) / RB;
  if (blocks > 2147483647LL) SP_FAIL("sp_trsm_rlt: too many rows");
  hipLaunchKernelGGL(trsm_rlt_kernel<T>, dim3((unsigned)blocks), dim3(RB), 0, st, L, ldl, n, B, ldb, m, info);
  SP_CHECK_LAUNCH();
  return 0;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int64_t up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// scratch a GEMM of the update may be handed: what its split-K wants -- unless the shape is one the bf16 split tier
// would take with that much scratch (the factorisation's error bound is stated for the plain fp32 / fp64 tiers)
size_t gemm_scratch(int32_t dtype, int64_t M, int64_t N, int64_t K) {
  if (sp_gemm_split_workspace_bytes(dtype, M, N, K) > 0) return 0;
  return sp_gemm_workspace_bytes(dtype, M, N, K);
}

// The GEMM updates of a factorisation of order n, in the order sp_potrf makes them: f(M, N, K).
template <typename F>
void for_each_update(int64_t n, F f) {
  for (int64_t j0 = 0; j0 < n; j0 += OB) {
    const int64_t w = (n - j0) < OB ? (n - j0) : OB;
    if (j0 > 0) f(n - j0, w, j0);
    for (int64_t i0 = NB; i0 < w; i0 += NB) f(n - j0 - i0, (w - i0) < NB ? (w - i0) : NB, i0);
  }
}

struct Scratch {
  size_t negt_bytes, gemm_bytes;
};

Scratch scratch_of(int32_t dtype, int64_t n) {
  Scratch s = {0, 0};
  const size_t es = sp_dtype_size(dtype);
  for_each_update(n, [&](int64_t M, int64_t N, int64_t K) {
    const size_t t = (size_t)K * (size_t)up4(N) * es, g = gemm_scratch(dtype, M, N, K);
    if (t > s.negt_bytes) s.negt_bytes = t;
    if (g > s.gemm_bytes) s.gemm_bytes = g;
  });
  return s;
}

// C[r0:n, r0:r0+N] += A[r0:n, c0:r0] . -(A[r0:r0+N, c0:r0])^T
template <typename T>
int update(int32_t dtype, T* A, int64_t lda, int64_t n, int64_t r0, int64_t c0, int64_t N, T* negt, void* gemm_ws,
           const int32_t* info, hipStream_t st) {
  const int64_t K = r0 - c0, M = n - r0, ldo = up4(N);
  hipLaunchKernelGGL(negt_kernel<T>, dim3((unsigned)((K + 31) / 32), (unsigned)((N + 31) / 32)), dim3(32, 8), 0, st,
                     A + r0 * lda + c0, lda, (int)N, K, negt, ldo, info);
  SP_CHECK_LAUNCH();
  const size_t g = gemm_scratch(dtype, M, N, K);
  return sp_gemm_ws(dtype, A + r0 * lda + c0, lda, negt, ldo, A + r0 * lda + r0, lda, M, N, K, 1, g ? gemm_ws : nullptr, g,
                    (void*)st);
}

template <typename T>
int potrf_run(int32_t dtype, T* A, int64_t lda, int64_t n, void* d_ws, int32_t* info, hipStream_t st) {
  const Scratch s = scratch_of(dtype, n);
  T* negt = (T*)up256((size_t)(uintptr_t)d_ws);
  void* gemm_ws = (void*)up256((size_t)(uintptr_t)negt + s.negt_bytes);
  for (int64_t j0 = 0; j0 < n; j0 += OB) {
    const int64_t w = (n - j0) < OB ? (n - j0) : OB;
    if (j0 > 0 && update<T>(dtype, A, lda, n, j0, 0, w, negt, gemm_ws, info, st)) return 1;
    for (int64_t i0 = 0; i0 < w; i0 += NB) {
      const int64_t r0 = j0 + i0, bw = (w - i0) < NB ? (w - i0) : NB;
      if (i0 > 0 && update<T>(dtype, A, lda, n, r0, j0, bw, negt, gemm_ws, info, st)) return 1;
      T* diag = A + r0 * lda + r0;
      hipLaunchKernelGGL(potrf_block_kernel<T>, dim3(1), dim3(256), 0, st, diag, lda, (int)bw, r0, info);
      SP_CHECK_LAUNCH();
      if (trsm_launch<T>(diag, lda, bw, diag + bw * lda, lda, n - r0 - bw, info, st)) return 1;
    }
  }
  if (n > 1) {
    hipLaunchKernelGGL(zero_upper_kernel<T>, dim3((unsigned)(n - 1)), dim3(256), 0, st, A, lda, n);
    SP_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" size_t sp_potrf_workspace_bytes(int32_t dtype, int64_t n) {
  if (n < 1 || (dtype != SP_F32 && dtype != SP_F64)) return 256;
  const Scratch s = scratch_of(dtype, n);
  return 256 + up256(s.negt_bytes) + 256 + s.gemm_bytes;
}

extern "C" int sp_potrf(int32_t dtype, void* d_A, int64_t lda, int64_t n, void* d_ws, size_t ws_bytes, int32_t* d_info,
                        void* stream) {
  if (dtype != SP_F32 && dtype != SP_F64)
    SP_FAIL("sp_potrf: dtype must be f32 or f64; convert with astype first");
  if (n < 0) SP_FAIL("sp_potrf: bad size");
  if (!d_info) SP_FAIL("sp_potrf: NULL info");
  hipStream_t st = (hipStream_t)stream;
  SP_HIP(hipMemsetAsync(d_info, 0, sizeof(int32_t), st));
  if (n == 0) return 0;
  if (n > 2147483647LL) SP_FAIL("sp_potrf: order too large");
  if (!d_A) SP_FAIL("sp_potrf: NULL pointer");
  if (lda < n) SP_FAIL("sp_potrf: leading dimension too small");
  if (n > NB && (!d_ws || ws_bytes < sp_potrf_workspace_bytes(dtype, n))) SP_FAIL("sp_potrf: workspace too small");
  if (dtype == SP_F32) return potrf_run<float>(dtype, (float*)d_A, lda, n, d_ws, d_info, st);
  return potrf_run<double>(dtype, (double*)d_A, lda, n, d_ws, d_info, st);
}

extern "C" int sp_trsm_rlt(int32_t dtype, const void* d_L, int64_t ldl, int64_t n, void* d_B, int64_t ldb, int64_t m,
                           void* stream) {
  if (dtype != SP_F32 && dtype != SP_F64)
    SP_FAIL("sp_trsm_rlt: dtype must be f32 or f64; convert with astype first");
  if (n < 0 || m < 0) SP_FAIL("sp_trsm_rlt: bad sizes");
  if (n == 0 || m == 0) return 0;
  if (!d_L || !d_B) SP_FAIL("sp_trsm_rlt: NULL pointer");
  if (ldl < n || ldb < n) SP_FAIL("sp_trsm_rlt: leading dimension too small");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SP_F32) return trsm_launch<float>((const float*)d_L, ldl, n, (float*)d_B, ldb, m, nullptr, st);
  return trsm_launch<double>((const double*)d_L, ldl, n, (double*)d_B, ldb, m, nullptr, st);
}
