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
#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_extras.h"
#include "../../include/spartan_hip_eig.h"

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
  T* negt = (T*)sp_align256((size_t)(uintptr_t)d_ws);
  void* gemm_ws = (void*)sp_align256((size_t)(uintptr_t)negt + s.negt_bytes);
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
  return 256 + sp_align256(s.negt_bytes) + 256 + s.gemm_bytes;
}

extern "C" int sp_potrf(int32_t dtype, void* d_A, int64_t lda, int64_t n, void* d_ws, size_t ws_bytes, int32_t* d_info,
                        void* stream) {
  return sp_float_dispatch("sp_potrf", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0) SP_FAIL("sp_potrf: bad size");
    if (!d_info) SP_FAIL("sp_potrf: NULL info");
    hipStream_t st = (hipStream_t)stream;
    SP_HIP(hipMemsetAsync(d_info, 0, sizeof(int32_t), st));
    if (n == 0) return 0;
    if (n > 2147483647LL) SP_FAIL("sp_potrf: order too large");
    if (!d_A) SP_FAIL("sp_potrf: NULL pointer");
    if (lda < n) SP_FAIL("sp_potrf: leading dimension too small");
    if (n > NB && (!d_ws || ws_bytes < sp_potrf_workspace_bytes(dtype, n))) SP_FAIL("sp_potrf: workspace too small");
    return potrf_run<T>(dtype, (T*)d_A, lda, n, d_ws, d_info, st);
  });
}

extern "C" int sp_trsm_rlt(int32_t dtype, const void* d_L, int64_t ldl, int64_t n, void* d_B, int64_t ldb, int64_t m,
                           void* stream) {
  return sp_float_dispatch("sp_trsm_rlt", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0 || m < 0) SP_FAIL("sp_trsm_rlt: bad sizes");
    if (n == 0 || m == 0) return 0;
    if (!d_L || !d_B) SP_FAIL("sp_trsm_rlt: NULL pointer");
    if (ldl < n || ldb < n) SP_FAIL("sp_trsm_rlt: leading dimension too small");
    return trsm_launch<T>((const T*)d_L, ldl, n, (T*)d_B, ldb, m, nullptr, (hipStream_t)stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// sp_syevj: the eigendecomposition of a symmetric tile, the np.linalg.eig of the reference's stochastic SVD
//   spartan/examples/ssvd/ssvd.py   (:36-38) S, U_ = np.linalg.eig(B . B^T) on the small K x K matrix; examples/pca.py
//
// Cyclic two-sided Jacobi, A <- J^T A J and V <- V J, the pairs of a sweep taken in the rounds of a round-robin
// tournament (the circle method): with m = n rounded up to even, round r of m - 1 pairs index m - 1 with r and every
// other index i with the i' for which i + i' = 2 r (mod m - 1); for odd n index m - 1 does not exist and its partner
// sits the round out.  The pairs of a round are disjoint, so their rotations commute as index sets: every element of
// J^T A J depends on the four elements at {i, i'} x {j, j'} and the two rotations, every element of V J on two.
// The rotation of the pair p < q is Rutishauser's: tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| +
// sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c, J = [c s; -s c]; a pair with a_pq == 0, or whose tau is not
// finite, or whose s underflows, is left alone.  Two deviations from the plain product: the rotated pair's own
// off-diagonal element is SET to zero (the classical one); and the four products of an element are added as
// (cc a + ss d) + (cs b + sc c), which is the same expression at (i, j) and (j, i), so that the iterate stays
// symmetric bit for bit and either triangle may be read.  (The other classical shortcut, the diagonal as a_pp - t a_pq
// and a_qq + t a_pq, is NOT taken: in a NumPy emulation of this arithmetic it left off(A) hovering at the threshold on
// the clustered input -- 44 sweeps at n = 65 in fp64, the cap at n = 257 -- where the product form needs 19 and 24.)
//
//   n <= 64 (fp32) / 63 (fp64): syevj_lds_kernel, one workgroup, A and V in LDS, in place (a thread owns whole
//       2 x 2 groups), two barriers per round, up to SYEVJ_LDS_SWEEPS sweeps per launch with the stop rule
//       evaluated in the kernel before every sweep;
//   above: syevj_round_kernel, one launch per round, out of place between two buffers of the workspace; every
//       workgroup works its 16 x 64 tile's 80 rotations out for itself from the diagonal of the round's input and
//       waits for no other.  syevj_off_kernel evaluates the stop rule once per sweep.
// The host reads one 8-byte word per sweep (per launch in LDS) and stops at off(A)_F <= n u ||A||_F or after
// SYEVJ_MAX_SWEEPS sweeps (then info = 1: a NaN never compares below the threshold and ends there).  No loop on the
// device depends on what another workgroup does.  syevj_sort_kernel ranks the diagonal by counting (ties by index)
// and gathers W and the columns of V into ascending order.
namespace {

constexpr int SYEVJ_MAX_SWEEPS = 64;  // the transcription in tests/eig_cases.py needs at most 26 on its inputs
constexpr int SYEVJ_LDS_SWEEPS = 8;   // sweeps one launch of the LDS kernel may run
constexpr int JC = 64, JR = 16;       // tile of one workgroup of the round kernel: JR rows of JC columns, block (64, 4)
constexpr int SYEVJ_MAX_ORDER = 32768;

template <typename T> struct SyevjLds;   // largest order held in LDS (A and V, 64 KiB of static LDS) and their row stride
template <> struct SyevjLds<float> { static constexpr int N = 64, LD = 65; };
template <> struct SyevjLds<double> { static constexpr int N = 63, LD = 64; };

struct SyevjWord {
  int32_t converged, sweeps;
};

template <typename T> struct Rot { T c, s; };

__device__ __forceinline__ float sp_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double sp_abs(double x) { return fabs(x); }
__device__ __forceinline__ float sp_sign1(float x) { return copysignf(1.0f, x); }
__device__ __forceinline__ double sp_sign1(double x) { return copysign(1.0, x); }
__device__ __forceinline__ double unit_roundoff(float) { return 5.9604644775390625e-08; }    // 2^-24
__device__ __forceinline__ double unit_roundoff(double) { return 1.1102230246251565e-16; }   // 2^-53
__device__ __forceinline__ float finite_max(float) { return 3.402823466e+38f; }
__device__ __forceinline__ double finite_max(double) { return 1.7976931348623157e+308; }

template <typename T>
__device__ __forceinline__ Rot<T> rotation(T app, T aqq, T apq) {
  Rot<T> r = {(T)1, (T)0};
  if (apq == (T)0) return r;
  const T tau = (aqq - app) / ((T)2 * apq);
  if (!(sp_abs(tau) <= finite_max(tau))) return r;      // overflow, or a NaN
  const T t = sp_sign1(tau) / (sp_abs(tau) + sp_sqrt_rn((T)1 + tau * tau));
  const T c = (T)1 / sp_sqrt_rn((T)1 + t * t);
  const T s = t * c;
  if (s == (T)0) return r;
  r.c = c;
  r.s = s;
  return r;
}

// partner of index i < m in round r < m - 1 (m even)
__device__ __forceinline__ int partner_of(int i, int r, int m) {
  const int m1 = m - 1;
  if (i == m1) return r;
  if (i == r) return m1;
  return (2 * r - i + m1) % m1;
}

// element (i, j) of J^T A J from a = A[i, j], b = A[i, j'], c = A[i', j], d = A[i', j']; (ci, si) and (cj, sj) are
// the cosine and the SIGNED sine of the index: -s for the smaller index of its pair, +s for the larger
template <typename T>
__device__ __forceinline__ T two_sided(T ci, T si, T cj, T sj, T a, T b, T c, T d) {
  return ((ci * cj) * a + (si * sj) * d) + ((ci * sj) * b + (si * cj) * c);
}

// sum of two doubles over the workgroup (whole waves, at most 16 of them), the same value in every thread; red: 32 doubles
__device__ __forceinline__ void block_sum2(double& x, double& y, double* red) {
  for (int d = 32; d > 0; d >>= 1) {
    x += __shfl_down(x, d, 64);
    y += __shfl_down(y, d, 64);
  }
  const int tid = threadIdx.y * blockDim.x + threadIdx.x, waves = (blockDim.x * blockDim.y) >> 6;
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = x;
    red[2 * (tid >> 6) + 1] = y;
  }
  __syncthreads();
  x = 0;
  y = 0;
  for (int w = 0; w < waves; ++w) {
    x += red[2 * w];
    y += red[2 * w + 1];
  }
  __syncthreads();
}

// the stop rule: off(A)_F <= n u ||A||_F, and false for anything that is not finite
template <typename T>
__device__ __forceinline__ bool stop_rule(double off2, double diag2, int n) {
  const double off = sqrt(off2), norm = sqrt(off2 + diag2);
  return off <= (double)n * unit_roundoff((T)0) * norm && norm <= finite_max(1.0);
}

template <typename T>
__global__ __launch_bounds__(256) void syevj_lds_kernel(const T* __restrict__ src, int64_t lda, int n, T* __restrict__ stA,
                                                        T* __restrict__ stV, int first, int max_sweeps, int sweeps_before,
                                                        SyevjWord* __restrict__ word) {
  constexpr int NM = SyevjLds<T>::N, LD = SyevjLds<T>::LD, HM = (NM + 1) / 2;
  __shared__ T SA[NM * LD], SV[NM * LD];
  __shared__ T rc[HM], rs[HM];
  __shared__ unsigned char rp[HM], rq[HM];      // the pair's smaller and larger index; rq = 255: nobody, the index sits out
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int m = n + (n & 1), h = m >> 1, rounds = m - 1;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e % n;
    if (first) {
      SA[i * LD + j] = i >= j ? src[(int64_t)i * lda + j] : src[(int64_t)j * lda + i];
      SV[i * LD + j] = i == j ? (T)1 : (T)0;
    } else {
      SA[i * LD + j] = stA[e];
      SV[i * LD + j] = stV[e];
    }
  }
  __syncthreads();
  int sweeps = 0;
  bool conv = false;
  for (;;) {                                     // at most max_sweeps + 1 trips
    double off2 = 0, diag2 = 0;
    for (int e = tid; e < n * n; e += 256) {
      const int i = e / n, j = e % n;
      const double v = (double)SA[i * LD + j];
      if (i == j) diag2 += v * v;
      else off2 += v * v;
    }
    block_sum2(off2, diag2, red);
    conv = stop_rule<T>(off2, diag2, n);
    if (conv || sweeps == max_sweeps) break;     // (the same in every thread)
    for (int r = 0; r < rounds; ++r) {
      if (tid < h) {
        int p, q;
        if (tid == 0) {
          p = r;
          q = m - 1;
        } else {
          const int x = (r + tid) % rounds, y = (r - tid + rounds) % rounds;
          p = x < y ? x : y;
          q = x < y ? y : x;
        }
        Rot<T> rot = {(T)1, (T)0};
        if (q < n) rot = rotation(SA[p * LD + p], SA[q * LD + q], SA[q * LD + p]);
        rp[tid] = (unsigned char)p;
        rq[tid] = (unsigned char)(q < n ? q : 255);
        rc[tid] = rot.c;
        rs[tid] = rot.s;
      }
      __syncthreads();
      for (int g = tid; g < h * h; g += 256) {   // A: the 2 x 2 group of pair ka's rows and pair kb's columns
        const int ka = g / h, kb = g % h;
        const int pa = rp[ka], qa = rq[ka], pb = rp[kb], qb = rq[kb];
        const bool ha = qa != 255, hb = qb != 255;
        const T ca = rc[ka], sa = rs[ka], cb = rc[kb], sb = rs[kb];
        const T a00 = SA[pa * LD + pb];
        const T a01 = hb ? SA[pa * LD + qb] : (T)0;
        const T a10 = ha ? SA[qa * LD + pb] : (T)0;
        const T a11 = ha && hb ? SA[qa * LD + qb] : (T)0;
        const T n00 = two_sided(ca, -sa, cb, -sb, a00, a01, a10, a11);
        T n01 = two_sided(ca, -sa, cb, sb, a01, a00, a11, a10);
        T n10 = two_sided(ca, sa, cb, -sb, a10, a11, a00, a01);
        const T n11 = two_sided(ca, sa, cb, sb, a11, a10, a01, a00);
        if (ka == kb && sa != (T)0) n01 = n10 = (T)0;    // the element the rotation annihilates
        SA[pa * LD + pb] = n00;
        if (hb) SA[pa * LD + qb] = n01;
        if (ha) SA[qa * LD + pb] = n10;
        if (ha && hb) SA[qa * LD + qb] = n11;
      }
      for (int g = tid; g < n * h; g += 256) {   // V: row i, the two columns of pair kb
        const int i = g / h, kb = g % h;
        const int pb = rp[kb], qb = rq[kb];
        if (qb == 255) continue;
        const T cb = rc[kb], sb = rs[kb];
        const T v0 = SV[i * LD + pb], v1 = SV[i * LD + qb];
        SV[i * LD + pb] = cb * v0 + (-sb) * v1;
        SV[i * LD + qb] = cb * v1 + sb * v0;
      }
      __syncthreads();
    }
    ++sweeps;
  }
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e % n;
    stA[e] = SA[i * LD + j];
    stV[e] = SV[i * LD + j];
  }
  if (tid == 0) {
    word->converged = conv ? 1 : 0;
    word->sweeps = sweeps_before + sweeps;
  }
}

// A0 <- the symmetric matrix whose lower triangle src holds, V0 <- I.  Block (64, 4), grid as the round kernel's.
template <typename T>
__global__ __launch_bounds__(256) void syevj_mirror_kernel(const T* __restrict__ src, int64_t lda, int n, T* __restrict__ A0,
                                                           T* __restrict__ V0) {
  const int j = blockIdx.x * JC + threadIdx.x;
  if (j >= n) return;
  for (int k = 0; k < JR / 4; ++k) {
    const int i = blockIdx.y * JR + threadIdx.y + 4 * k;
    if (i >= n) return;
    A0[(int64_t)i * n + j] = i >= j ? src[(int64_t)i * lda + j] : src[(int64_t)j * lda + i];
    V0[(int64_t)i * n + j] = i == j ? (T)1 : (T)0;
  }
}

// One round, out of place: B = J^T A J, Vn = V J (all four n x n, contiguous).  Block (64, 4).
template <typename T>
__global__ __launch_bounds__(256) void syevj_round_kernel(const T* __restrict__ A, T* __restrict__ B, const T* __restrict__ V,
                                                          T* __restrict__ Vn, int n, int m, int r) {
  __shared__ T rc[JC + JR], rs[JC + JR];
  __shared__ int rp[JC + JR];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
  const int j0 = blockIdx.x * JC, i0 = blockIdx.y * JR;
  if (tid < JC + JR) {          // the tile's columns, then its rows
    const int i = tid < JC ? j0 + tid : i0 + tid - JC;
    T c = (T)1, s = (T)0;
    int ip = i;
    if (i < n) {
      const int k = partner_of(i, r, m);
      if (k < n) {
        const int64_t p = i < k ? i : k, q = i < k ? k : i;
        const Rot<T> rot = rotation(A[p * n + p], A[q * n + q], A[q * n + p]);
        ip = k;
        c = rot.c;
        s = i == p ? -rot.s : rot.s;
      }
    }
    rc[tid] = c;
    rs[tid] = s;
    rp[tid] = ip;
  }
  __syncthreads();
  const int j = j0 + tx;
  if (j >= n) return;
  const T cj = rc[tx], sj = rs[tx];
  const int jp = rp[tx];
  for (int k = 0; k < JR / 4; ++k) {
    const int li = ty + 4 * k, i = i0 + li;
    if (i >= n) return;
    const T ci = rc[JC + li], si = rs[JC + li];
    const int ip = rp[JC + li];
    const T* row = A + (int64_t)i * n;
    const T* rowp = A + (int64_t)ip * n;
    const T a = row[j], b = row[jp], c = rowp[j], d = rowp[jp];
    T val = two_sided(ci, si, cj, sj, a, b, c, d);
    if (j == ip && j != i && si != (T)0) val = (T)0;     // the element the rotation annihilates
    B[(int64_t)i * n + j] = val;
    const T* vrow = V + (int64_t)i * n;
    Vn[(int64_t)i * n + j] = cj * vrow[j] + sj * vrow[jp];
  }
}

// The stop rule on the n x n iterate: one workgroup of 1024 threads.
template <typename T>
__global__ __launch_bounds__(1024) void syevj_off_kernel(const T* __restrict__ A, int n, SyevjWord* __restrict__ word) {
  __shared__ double red[32];
  double off2 = 0, diag2 = 0;
  for (int i = threadIdx.x >> 6; i < n; i += 16) {        // a wave per row
    const T* row = A + (int64_t)i * n;
    for (int j = threadIdx.x & 63; j < n; j += 64) {
      const double v = (double)row[j];
      if (i == j) diag2 += v * v;
      else off2 += v * v;
    }
  }
  block_sum2(off2, diag2, red);
  if (threadIdx.x == 0) word->converged = stop_rule<T>(off2, diag2, n) ? 1 : 0;
}

// W[rank(j)] = A[j, j], Vout[:, rank(j)] = V[:, j] with rank(j) the number of diagonal elements below a_jj (equal
// ones: with a smaller index); *info = failed.  Block (64, 4), grid as the round kernel's.
template <typename T>
__global__ __launch_bounds__(256) void syevj_sort_kernel(const T* __restrict__ A, const T* __restrict__ V, int n,
                                                         T* __restrict__ W, T* __restrict__ Vout, int64_t ldv,
                                                         int32_t* __restrict__ info, int32_t failed) {
  __shared__ int part[4][JC];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int j = blockIdx.x * JC + tx;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tx == 0 && ty == 0) *info = failed;
  int count = 0;
  T dj = (T)0;
  if (j < n) {
    dj = A[(int64_t)j * n + j];
    for (int k = ty; k < n; k += 4) {
      const T dk = A[(int64_t)k * n + k];
      count += (dk < dj || (dk == dj && k < j)) ? 1 : 0;
    }
  }
  part[ty][tx] = count;
  __syncthreads();
  if (j >= n) return;
  const int rank = part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx];    // < n whatever the values are
  if (blockIdx.y == 0 && ty == 0) W[rank] = dj;
  for (int k = 0; k < JR / 4; ++k) {
    const int i = blockIdx.y * JR + ty + 4 * k;
    if (i >= n) return;
    Vout[(int64_t)i * ldv + rank] = V[(int64_t)i * n + j];
  }
}

size_t syevj_buffer_bytes(int32_t dtype, int64_t n) { return sp_align256((size_t)n * (size_t)n * sp_dtype_size(dtype)); }

template <typename T>
int syevj_read_word(const SyevjWord* d_word, SyevjWord* h, hipStream_t st) {
  SP_HIP(hipMemcpyAsync(h, d_word, sizeof(SyevjWord), hipMemcpyDeviceToHost, st));
  SP_HIP(hipStreamSynchronize(st));
  return 0;
}

template <typename T>
int syevj_run(int32_t dtype, const T* A, int64_t lda, int n, T* W, T* V, int64_t ldv, void* d_ws, int32_t* info,
              int32_t* sweeps_out, hipStream_t st) {
  char* base = (char*)sp_align256((size_t)(uintptr_t)d_ws);
  SyevjWord* word = (SyevjWord*)base;
  const size_t nn = syevj_buffer_bytes(dtype, n);
  T* bufA[2] = {(T*)(base + 256), (T*)(base + 256 + 2 * nn)};
  T* bufV[2] = {(T*)(base + 256 + nn), (T*)(base + 256 + 3 * nn)};
  const int m = n + (n & 1);
  const dim3 grid((unsigned)((n + JC - 1) / JC), (unsigned)((n + JR - 1) / JR)), block(64, 4);
  SyevjWord h = {0, 0};
  int cur = 0, sweeps = 0;
  if (n <= SyevjLds<T>::N) {
    for (int launch = 0; launch < SYEVJ_MAX_SWEEPS / SYEVJ_LDS_SWEEPS && !h.converged; ++launch) {
      hipLaunchKernelGGL(syevj_lds_kernel<T>, dim3(1), dim3(256), 0, st, launch == 0 ? A : (const T*)bufA[0],
                         launch == 0 ? lda : (int64_t)n, n, bufA[0], bufV[0], launch == 0 ? 1 : 0, SYEVJ_LDS_SWEEPS,
                         launch * SYEVJ_LDS_SWEEPS, word);
      SP_CHECK_LAUNCH();
      if (syevj_read_word<T>(word, &h, st)) return 1;
      sweeps = h.sweeps;
    }
  } else {
    hipLaunchKernelGGL(syevj_mirror_kernel<T>, grid, block, 0, st, A, lda, n, bufA[0], bufV[0]);
    SP_CHECK_LAUNCH();
    for (;;) {                                            // at most SYEVJ_MAX_SWEEPS + 1 trips
      hipLaunchKernelGGL(syevj_off_kernel<T>, dim3(1), dim3(1024), 0, st, (const T*)bufA[cur], n, word);
      SP_CHECK_LAUNCH();
      if (syevj_read_word<T>(word, &h, st)) return 1;
      if (h.converged || sweeps == SYEVJ_MAX_SWEEPS) break;
      for (int r = 0; r < m - 1; ++r, cur ^= 1) {
        hipLaunchKernelGGL(syevj_round_kernel<T>, grid, block, 0, st, (const T*)bufA[cur], bufA[cur ^ 1],
                           (const T*)bufV[cur], bufV[cur ^ 1], n, m, r);
        SP_CHECK_LAUNCH();
      }
      ++sweeps;
    }
  }
  hipLaunchKernelGGL(syevj_sort_kernel<T>, grid, block, 0, st, (const T*)bufA[cur], (const T*)bufV[cur], n, W, V, ldv, info,
                     h.converged ? 0 : 1);
  SP_CHECK_LAUNCH();
  if (sweeps_out) *sweeps_out = sweeps;
  return 0;
}

}  // namespace

extern "C" size_t sp_syevj_workspace_bytes(int32_t dtype, int64_t n) {
  if (n < 1 || n > SYEVJ_MAX_ORDER || (dtype != SP_F32 && dtype != SP_F64)) return 512;
  const int lds = dtype == SP_F32 ? SyevjLds<float>::N : SyevjLds<double>::N;
  return 512 + (n <= lds ? 2 : 4) * syevj_buffer_bytes(dtype, n);
}

extern "C" int sp_syevj(int32_t dtype, void* d_A, int64_t lda, int64_t n, void* d_W, void* d_V, int64_t ldv, void* d_ws,
                        size_t ws_bytes, int32_t* d_info, int32_t* sweeps_out, void* stream) {
  return sp_float_dispatch("sp_syevj", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0) SP_FAIL("sp_syevj: bad size");
    if (!d_info) SP_FAIL("sp_syevj: NULL info");
    hipStream_t st = (hipStream_t)stream;
    SP_HIP(hipMemsetAsync(d_info, 0, sizeof(int32_t), st));
    if (sweeps_out) *sweeps_out = 0;
    if (n == 0) return 0;
    if (n > SYEVJ_MAX_ORDER) SP_FAIL("sp_syevj: order too large for the Jacobi solver");
    if (!d_A || !d_W || !d_V) SP_FAIL("sp_syevj: NULL pointer");
    if (lda < n || ldv < n) SP_FAIL("sp_syevj: leading dimension too small");
    if (!d_ws || ws_bytes < sp_syevj_workspace_bytes(dtype, n)) SP_FAIL("sp_syevj: workspace too small");
    return syevj_run<T>(dtype, (const T*)d_A, lda, (int)n, (T*)d_W, (T*)d_V, ldv, d_ws, d_info, sweeps_out, st);
  });
}
