// All-pairs shortest paths as a blocked Floyd-Warshall, and the dense graph of a neighbour list: the geodesic step of the
// reference's Isomap
//   spartan/examples/sklearn/manifold/isomap.py          (the neighbour graph, then shortest paths, then the kernel's eigenvectors)
//   spartan/examples/sklearn/util/graph_shortest_path.pyx  (there: Dijkstra on a Fibonacci heap, one source row at a time)
// The contract is in include/spartan_hip_graph.h.  Blocks of BS = 64; round kb is three launches:
//   apsp_diag_kernel    one workgroup: block (kb, kb) closes on itself in LDS, 64 dependent steps.
//   apsp_panel_kernel   2 (nb - 1) workgroups: the blocks of block row kb, C <- min(C, A (x) C) with A the closed diagonal
//                       block, and of block column kb, C <- min(C, C (x) A).  Step k needs row k of C as steps 0 .. k - 1
//                       left it: the patch lives in registers, the one row the next step reads goes back to LDS, one
//                       barrier per step.  A column block is the same computation on C^T and A^T: it is transposed on
//                       its way into LDS and on its way out, and the kernel has one body.
//   apsp_outer_kernel   (nb - 1)^2 workgroups: C <- min(C, A (x) B), A = D[i, kb], B = D[kb, j].  The n^3 part: its 64 steps
//                       are independent.  A goes into LDS k-major (At[k][i]), B as it is (Bs[k][j]), rows PITCH = 68
//                       elements apart, so that thread (ty, tx) of the 16 x 16 grid reads its four A values and its four B
//                       values of step k as one 16-byte-aligned vector each (a 16-lane group of the wide LDS read
//                       sees one A address -- a broadcast -- and 16 consecutive B slots); 16 adds and 16 mins follow,
//                       two steps at a time so that min(min(c, t1), t2) is one three-operand min.  No barrier in the loop.
// min, not compare-select: without NaN (info = 1 otherwise) fmin(c, t) is c unless t < c, the rule of the contract.
// Everything in one block of (x) is padded with +inf in LDS where the matrix ends; stores are guarded.
#include <limits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_graph.h"

namespace {

constexpr int BS = 64;        // block size
constexpr int PITCH = 68;     // elements between the rows of a staged block (BS + 4: 16-byte aligned rows)

template <typename T>
__device__ __forceinline__ T inf_of() {
  return std::numeric_limits<T>::infinity();
}

__device__ __forceinline__ float min_of(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_of(double a, double b) { return __builtin_fmin(a, b); }

// info <- 1 if an off-diagonal entry is NaN or negative; the diagonal <- 0
template <typename T>
__global__ __launch_bounds__(256) void apsp_check_kernel(T* __restrict__ D, int64_t ldd, int64_t n,
                                                         int32_t* __restrict__ info) {
  const int64_t total = n * n;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / n, j = e - i * n;
    if (i == j) D[i * ldd + j] = (T)0;
    else bad = bad || !(D[i * ldd + j] >= (T)0);
  }
  if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) *info = 1;       // (every writer stores the same word)
}

// block (r0, r0), bw x bw of it inside the matrix
template <typename T>
__global__ __launch_bounds__(256) void apsp_diag_kernel(T* __restrict__ D, int64_t ldd, int64_t r0, int bw) {
  __shared__ __attribute__((aligned(16))) T cs[BS * PITCH];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  T* blk = D + r0 * ldd + r0;
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e >> 6, c = e & 63;
    cs[r * PITCH + c] = (r < bw && c < bw) ? blk[(int64_t)r * ldd + c] : inf_of<T>();
  }
  __syncthreads();
  T acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(cs + (ty * 4 + a) * PITCH + tx * 4);
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = v.v[b];
  }
  for (int k = 0; k < BS; ++k) {
    T col[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) col[a] = cs[(ty * 4 + a) * PITCH + k];
    const Vec4<T> row = *reinterpret_cast<const Vec4<T>*>(cs + k * PITCH + tx * 4);
    __syncthreads();                    // row k and column k as steps 0 .. k - 1 left them are in registers everywhere
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      Vec4<T> out;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        acc[a][b] = min_of(acc[a][b], col[a] + row.v[b]);
        out.v[b] = acc[a][b];
      }
      *reinterpret_cast<Vec4<T>*>(cs + (ty * 4 + a) * PITCH + tx * 4) = out;
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int r = ty * 4 + a, c = tx * 4 + b;
      if (r < bw && c < bw) blk[(int64_t)r * ldd + c] = acc[a][b];
    }
}

// Workgroups 0 .. nb - 2: block (kb, j) of block row kb; nb - 1 .. 2 nb - 3: block (i, kb) of block column kb (j, i skip kb).
template <typename T>
__global__ __launch_bounds__(256) void apsp_panel_kernel(T* __restrict__ D, int64_t ldd, int64_t n, int kb, int nb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char apsp_smem[];
  T* at = reinterpret_cast<T*>(apsp_smem);       // [BS][PITCH]: at[k][i] = A[i][k] (row block) | A[k][i] (column block)
  T* cs = at + BS * PITCH;                       // [BS][PITCH]: C (row block) | C^T (column block)
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const bool column = (int)blockIdx.x >= nb - 1;
  int other = column ? (int)blockIdx.x - (nb - 1) : (int)blockIdx.x;
  if (other >= kb) ++other;
  const int64_t k0 = (int64_t)kb * BS, o0 = (int64_t)other * BS;
  const int kw = (int)(n - k0 < BS ? n - k0 : BS), ow = (int)(n - o0 < BS ? n - o0 : BS);
  const T* diag = D + k0 * ldd + k0;
  // the block in global memory: rows x cols = kw x ow (row block) | ow x kw (column block)
  T* blk = column ? D + o0 * ldd + k0 : D + k0 * ldd + o0;
  const int rows = column ? ow : kw, cols = column ? kw : ow;
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e >> 6, c = e & 63;
    const T a = (r < kw && c < kw) ? diag[(int64_t)r * ldd + c] : inf_of<T>();
    const T v = (r < rows && c < cols) ? blk[(int64_t)r * ldd + c] : inf_of<T>();
    if (column) {
      at[r * PITCH + c] = a;
      cs[c * PITCH + r] = v;
    } else {
      at[c * PITCH + r] = a;
      cs[r * PITCH + c] = v;
    }
  }
  __syncthreads();
  T acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const Vec4<T> v = *reinterpret_cast<const Vec4<T>*>(cs + (ty * 4 + a) * PITCH + tx * 4);
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = v.v[b];
  }
  // (row 0 of cs is read by step 0 as it was staged; row k + 1 is stored by its owner after step k.  Row k itself does
  // not change in step k: A[k][k] = 0, and a padded row is +inf throughout)
  for (int kk = 0; kk < BS / 4; ++kk) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = kk * 4 + s;
      const Vec4<T> av = *reinterpret_cast<const Vec4<T>*>(at + k * PITCH + ty * 4);
      const Vec4<T> cv = *reinterpret_cast<const Vec4<T>*>(cs + k * PITCH + tx * 4);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = min_of(acc[a][b], av.v[a] + cv.v[b]);
      const int next = k + 1;                    // row `next` = patch row (s + 1) & 3 of the threads with ty = next >> 2
      if (ty == (next >> 2)) {
        Vec4<T> out;
#pragma unroll
        for (int b = 0; b < 4; ++b) out.v[b] = acc[(s + 1) & 3][b];
        *reinterpret_cast<Vec4<T>*>(cs + next * PITCH + tx * 4) = out;
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    Vec4<T> out;
#pragma unroll
    for (int b = 0; b < 4; ++b) out.v[b] = acc[a][b];
    *reinterpret_cast<Vec4<T>*>(cs + (ty * 4 + a) * PITCH + tx * 4) = out;
  }
  __syncthreads();
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e >> 6, c = e & 63;
    if (r < rows && c < cols) blk[(int64_t)r * ldd + c] = column ? cs[c * PITCH + r] : cs[r * PITCH + c];
  }
}

// Workgroup (x, y): block (i, j) with i = y, j = x, both skipping kb.
template <typename T>
__global__ __launch_bounds__(256) void apsp_outer_kernel(T* __restrict__ D, int64_t ldd, int64_t n, int kb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char apsp_smem[];
  T* at = reinterpret_cast<T*>(apsp_smem);       // [BS][PITCH]: at[k][i] = A[i][k]
  T* bs = at + BS * PITCH;                       // [BS][PITCH]: bs[k][j] = B[k][j]
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int bi = (int)blockIdx.y + ((int)blockIdx.y >= kb ? 1 : 0), bj = (int)blockIdx.x + ((int)blockIdx.x >= kb ? 1 : 0);
  const int64_t k0 = (int64_t)kb * BS, i0 = (int64_t)bi * BS, j0 = (int64_t)bj * BS;
  const int kw = (int)(n - k0 < BS ? n - k0 : BS), iw = (int)(n - i0 < BS ? n - i0 : BS),
            jw = (int)(n - j0 < BS ? n - j0 : BS);
  const T* A = D + i0 * ldd + k0;
  const T* B = D + k0 * ldd + j0;
  T* Cb = D + i0 * ldd + j0;
  // A: thread (lr + 16 p, lc + 16 q): 16 consecutive lanes read 16 consecutive k of one row, and the transposed store
  // at[k][i] of a wave falls on 64 different banks; B: a wave reads and stores one whole row
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = ty + 16 * p, c = tx + 16 * q;
      at[c * PITCH + r] = (r < iw && c < kw) ? A[(int64_t)r * ldd + c] : inf_of<T>();
    }
  for (int e = tid; e < BS * BS; e += 256) {
    const int r = e >> 6, c = e & 63;
    bs[r * PITCH + c] = (r < kw && c < jw) ? B[(int64_t)r * ldd + c] : inf_of<T>();
  }
  T acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int r = ty * 4 + a, c = tx * 4 + b;
      acc[a][b] = (r < iw && c < jw) ? Cb[(int64_t)r * ldd + c] : inf_of<T>();
    }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < BS; k += 2) {
    const Vec4<T> a0 = *reinterpret_cast<const Vec4<T>*>(at + k * PITCH + ty * 4);
    const Vec4<T> b0 = *reinterpret_cast<const Vec4<T>*>(bs + k * PITCH + tx * 4);
    const Vec4<T> a1 = *reinterpret_cast<const Vec4<T>*>(at + (k + 1) * PITCH + ty * 4);
    const Vec4<T> b1 = *reinterpret_cast<const Vec4<T>*>(bs + (k + 1) * PITCH + tx * 4);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        acc[a][b] = min_of(min_of(acc[a][b], a0.v[a] + b0.v[b]), a1.v[a] + b1.v[b]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int r = ty * 4 + a, c = tx * 4 + b;
      if (r < iw && c < jw) Cb[(int64_t)r * ldd + c] = acc[a][b];
    }
}

template <typename T>
int apsp_run(T* D, int64_t ldd, int64_t n, int32_t* info, hipStream_t st) {
  const int64_t total = n * n;
  int64_t blocks = (total + 255) / 256;
  if (blocks > SP_CUS * SP_BLOCKS_PER_CU) blocks = SP_CUS * SP_BLOCKS_PER_CU;
  hipLaunchKernelGGL(apsp_check_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, D, ldd, n, info);
  SP_CHECK_LAUNCH();
  const int64_t nb = (n + BS - 1) / BS;
  const size_t lds = 2 * (size_t)BS * PITCH * sizeof(T);
  if (nb > 1) {
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(apsp_panel_kernel<T>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(apsp_outer_kernel<T>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  for (int64_t kb = 0; kb < nb; ++kb) {
    const int64_t r0 = kb * BS;
    const int bw = (int)(n - r0 < BS ? n - r0 : BS);
    hipLaunchKernelGGL(apsp_diag_kernel<T>, dim3(1), dim3(256), 0, st, D, ldd, r0, bw);
    SP_CHECK_LAUNCH();
    if (nb == 1) break;
    hipLaunchKernelGGL(apsp_panel_kernel<T>, dim3((unsigned)(2 * (nb - 1))), dim3(256), lds, st, D, ldd, n, (int)kb, (int)nb);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(apsp_outer_kernel<T>, dim3((unsigned)(nb - 1), (unsigned)(nb - 1)), dim3(256), lds, st, D, ldd, n,
                       (int)kb);
    SP_CHECK_LAUNCH();
  }
  return 0;
}

// W <- +inf, 0 on the diagonal
template <typename T>
__global__ __launch_bounds__(256) void graph_fill_kernel(T* __restrict__ W, int64_t ldw, int64_t n) {
  const int64_t total = n * n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / n, j = e - i * n;
    W[i * ldw + j] = i == j ? (T)0 : inf_of<T>();
  }
}

__device__ __forceinline__ void min_bits(float* p, float v) {
  atomicMin(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void min_bits(double* p, double v) {
  atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v));
}

// one thread per listed pair.  Non-negative floats order as their bit patterns do (unsigned); a negative weight or a
// NaN has a pattern above +inf's or is not below it and never wins.
template <typename T>
__global__ __launch_bounds__(256) void graph_scatter_kernel(const T* __restrict__ dist, const int64_t* __restrict__ idx,
                                                            int64_t ldk, int64_t n, int64_t k, T* __restrict__ W,
                                                            int64_t ldw) {
  const int64_t total = n * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / k, s = e - i * k;
    const int64_t j = idx[i * ldk + s];
    if (j < 0 || j >= n || j == i) continue;
    const T w = dist[i * ldk + s];
    min_bits(W + i * ldw + j, w);
    min_bits(W + j * ldw + i, w);
  }
}

template <typename T>
int graph_run(const T* dist, const int64_t* idx, int64_t ldk, int64_t n, int64_t k, T* W, int64_t ldw, hipStream_t st) {
  const int64_t cap = SP_CUS * SP_BLOCKS_PER_CU;
  int64_t blocks = (n * n + 255) / 256;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(graph_fill_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, W, ldw, n);
  SP_CHECK_LAUNCH();
  if (k == 0) return 0;
  blocks = (n * k + 255) / 256;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(graph_scatter_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, dist, idx, ldk, n, k, W, ldw);
  SP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sp_apsp(int32_t dtype, void* d_D, int64_t ldd, int64_t n, int32_t* d_info, void* stream) {
  return sp_float_dispatch("sp_apsp", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0 || ldd < n) SP_FAIL("sp_apsp: bad shape n=%lld ldd=%lld", (long long)n, (long long)ldd);
    if (n > 65535LL * BS) SP_FAIL("sp_apsp: order %lld is too large (at most %lld)", (long long)n, 65535LL * BS);
    if (!d_info) SP_FAIL("sp_apsp: NULL info");
    hipStream_t st = (hipStream_t)stream;
    SP_HIP(hipMemsetAsync(d_info, 0, sizeof(int32_t), st));
    if (n == 0) return 0;
    return apsp_run<T>((T*)d_D, ldd, n, d_info, st);
  });
}

extern "C" int sp_graph_from_knn(int32_t dtype, const void* d_dist, const int64_t* d_idx, int64_t ldk, int64_t n,
                                 int64_t k, void* d_W, int64_t ldw, void* stream) {
  return sp_float_dispatch("sp_graph_from_knn", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0 || k < 0 || ldk < k || ldw < n)
      SP_FAIL("sp_graph_from_knn: bad shape n=%lld k=%lld ldk=%lld ldw=%lld", (long long)n, (long long)k, (long long)ldk,
              (long long)ldw);
    if (n > 0x7fffffffLL / 2) SP_FAIL("sp_graph_from_knn: order %lld is too large", (long long)n);
    if (n == 0) return 0;
    return graph_run<T>((const T*)d_dist, d_idx, ldk, n, k, (T*)d_W, ldw, (hipStream_t)stream);
  });
}
