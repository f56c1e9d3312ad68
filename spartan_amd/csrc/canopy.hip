// The two tile bodies of the reference's canopy clustering:
//   spartan/examples/canopy_clustering.py   _canopy_mapper (:33-65: a loop over the rows and, inside it, a loop over the
//                                           canopies found so far)
//                                           _cluster_mapper (:68-92: the first centre of largest 1 / (1 + dist) per row)
// The contract is in include/spartan_hip_canopy.h.  Two kernels:
//   canopy_kernel     a workgroup of 256 threads per chain, rows in blocks of 64.  Everything order-dependent in a block
//                     is 64 steps of scalar bit arithmetic in one wave; the distances that feed it are 64 x 64 tiles
//                     (sp_d2_tile) and the sums are added by a thread per (canopy, feature) in ascending row order.
//   pdf_label_kernel  a workgroup of 256 threads per 64 rows, the centres 64 at a time (sp_d2_tile).
#include <cmath>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_canopy.h"

namespace {

typedef unsigned long long cn_mask;     // a bit per row of a block of 64

// a wave-uniform mask out of lane `k` of a register
__device__ __forceinline__ cn_mask cn_lane_value(cn_mask v, int k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
  return ((cn_mask)hi << 32) | lo;
}

// s + the rows r0 + i of X, feature f, for the bits i of `mask` ascending: one add each.  (Eight loads at a time ahead
// of their additions was measured: 5 % faster on the reference's benchmark, 11 % slower with thousands of canopies.)
template <typename T>
__device__ __forceinline__ T cn_add_rows(T s, cn_mask mask, const T* __restrict__ X, int64_t ldx, int64_t r0, int64_t f) {
  while (mask) {
    const int i = __builtin_ctzll(mask);
    mask &= mask - 1;
    s = s + X[(r0 + i) * ldx + f];
  }
  return s;
}

// W (the creating rows), S (the sums, then the means), cnt and crow are this chain's slots: read and written by this
// workgroup alone, every write a barrier ahead of the reads of another thread.
template <typename T>
__global__ __launch_bounds__(256) void canopy_kernel(const T* __restrict__ X, int64_t ldx, int64_t n, int64_t d, T t1, T t2,
                                                     int64_t chains, int64_t cap, T* centers, int64_t ldc, int64_t* counts,
                                                     int64_t* rows, int64_t* num, T* ws) {
  __shared__ __attribute__((aligned(16))) T xs[SP_D2_DC * SP_D2_PITCH];
  __shared__ __attribute__((aligned(16))) T cs[SP_D2_DC * SP_D2_PITCH];
  __shared__ cn_mask s_near[64];        // row i of the block: the earlier rows of the block within t2
  __shared__ cn_mask s_later[64];       // row j of the block: the later rows of the block within t1
  __shared__ cn_mask s_obs[64];         // canopy j of this tile of 64 canopies: the block's rows within t1
  __shared__ cn_mask s_bound;           // the block's rows within t2 of a canopy made before the block
  __shared__ cn_mask s_new;             // the block's rows that become canopies
  __shared__ int s_list[64];            // ... their numbers in the block, ascending

  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t c = blockIdx.x;
  const int64_t row_b = c * n / chains, row_e = (c + 1) * n / chains;
  T* W = ws + c * cap * d;
  T* S = centers + c * cap * ldc;
  int64_t* cnt = counts + c * cap;
  int64_t* crow = rows + c * cap;
  int64_t m = 0;                        // canopies so far (the same in every thread)
  T acc[4][4];

  for (int64_t r0 = row_b; r0 < row_e; r0 += 64) {
    const int nb = (int)(row_e - r0 < 64 ? row_e - r0 : 64);
    if (tid < 64) {
      s_near[tid] = 0;
      s_later[tid] = 0;
    }
    if (tid == 0) s_bound = 0;

    // the block against the canopies made before it, 64 at a time (the tile's barriers order the zeros above and
    // below ahead of the bit operations)
    for (int64_t c0 = 0; c0 < m; c0 += 64) {
      if (tid < 64) s_obs[tid] = 0;
      sp_d2_tile<T>(X, ldx, row_e, r0, W, d, m, c0, d, xs, cs, tid, acc);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = ty * 4 + a, j = tx * 4 + b;
          if (i < nb && c0 + j < m) {
            if (acc[a][b] < t2) atomicOr(&s_bound, (cn_mask)1 << i);
            if (acc[a][b] < t1) atomicOr(&s_obs[j], (cn_mask)1 << i);
          }
        }
      __syncthreads();
      const int nc = (int)(m - c0 < 64 ? m - c0 : 64);
      if (tid < nc && s_obs[tid]) cnt[c0 + tid] += __popcll(s_obs[tid]);
      for (int64_t e = tid; e < nc * d; e += 256) {
        const int64_t j = e / d, f = e - j * d;
        const cn_mask mask = s_obs[j];
        if (mask) S[(c0 + j) * ldc + f] = cn_add_rows(S[(c0 + j) * ldc + f], mask, X, ldx, r0, f);
      }
      __syncthreads();
    }

    // the block against itself: (i, j) with j < i, both rows of the chain
    sp_d2_tile<T>(X, ldx, row_e, r0, X, ldx, row_e, r0, d, xs, cs, tid, acc);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = ty * 4 + a, j = tx * 4 + b;
        if (j < i && i < nb) {
          if (acc[a][b] < t2) atomicOr(&s_near[i], (cn_mask)1 << j);
          if (acc[a][b] < t1) atomicOr(&s_later[j], (cn_mask)1 << i);
        }
      }
    __syncthreads();

    // the block in order: row i becomes a canopy unless it is bound or an earlier NEW row is within t2 (everything
    // here is the same in all lanes of the one wave)
    if (tid < 64) {
      const cn_mask mine = s_near[tid], bound = s_bound;
      cn_mask fresh = 0;
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        const cn_mask near_i = cn_lane_value(mine, i);
        const bool is_new = i < nb && !((bound >> i) & 1) && !(near_i & fresh);
        fresh |= (cn_mask)is_new << i;
      }
      if ((fresh >> tid) & 1) s_list[__popcll(fresh & (((cn_mask)1 << tid) - 1))] = tid;
      if (tid == 0) s_new = fresh;
    }
    __syncthreads();
    const int nn = __popcll(s_new);
    if (m + nn > cap) {                 // (the same for the whole workgroup)
      if (tid == 0) num[c] = -1;
      return;
    }
    if (tid < nn) {
      const int i = s_list[tid];
      cnt[m + tid] = 1 + __popcll(s_later[i]);
      crow[m + tid] = r0 + i;
    }
    for (int64_t e = tid; e < nn * d; e += 256) {
      const int64_t q = e / d, f = e - q * d;
      const int i = s_list[q];
      const T x = X[(r0 + i) * ldx + f];
      W[(m + q) * d + f] = x;
      S[(m + q) * ldc + f] = cn_add_rows(x, s_later[i], X, ldx, r0, f);
    }
    m += nn;
    __syncthreads();
  }

  for (int64_t e = tid; e < m * d; e += 256) {
    const int64_t j = e / d, f = e - j * d;
    S[j * ldc + f] = S[j * ldc + f] / (T)cnt[j];
  }
  if (tid == 0) num[c] = m;
}

template <typename T>
__global__ __launch_bounds__(256) void pdf_label_kernel(const T* __restrict__ X, int64_t ldx, int64_t n,
                                                        const T* __restrict__ C, int64_t ldc, int64_t k, int64_t d,
                                                        int32_t* __restrict__ labels) {
  __shared__ __attribute__((aligned(16))) T xs[SP_D2_DC * SP_D2_PITCH];
  __shared__ __attribute__((aligned(16))) T cs[SP_D2_DC * SP_D2_PITCH];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  T best[4], acc[4][4];
  int32_t at[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    best[a] = (T)-1;
    at[a] = -1;
  }
  for (int64_t c0 = 0; c0 < k; c0 += 64) {
    sp_d2_tile<T>(X, ldx, n, r0, C, ldc, k, c0, d, xs, cs, tid, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b) {       // (this thread's centres ascending: strict <, the first of equals stays)
      const int64_t j = c0 + tx * 4 + b;
      if (j < k) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const T pdf = (T)1 / ((T)1 + acc[a][b]);
          if (best[a] < pdf) {
            best[a] = pdf;
            at[a] = (int32_t)j;
          }
        }
      }
    }
  }
  // the 16 threads of a row (consecutive lanes): larger pdf, then lower index; (-1, -1) loses to every real pdf >= 0
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
      const T op = __shfl_xor(best[a], s);
      const int32_t oi = __shfl_xor(at[a], s);
      if (best[a] < op || (best[a] == op && oi < at[a])) {
        best[a] = op;
        at[a] = oi;
      }
    }
    const int64_t r = r0 + ty * 4 + a;
    if (tx == 0 && r < n) labels[r] = at[a];
  }
}

// what both entry points of sp_canopy refuse about the sizes
bool canopy_sizes_ok(int64_t n, int64_t d, int64_t chains, int64_t cap, int64_t ld) {
  if (n < 0 || d < 1 || chains < 1 || cap < 1 || ld < d) return false;
  if (chains > 0x7fffffffLL || (double)chains * (double)(n > 0 ? n : 1) > 4.0e18) return false;
  return (double)chains * (double)cap * (double)ld <= 1.0e17;
}

}  // namespace

extern "C" size_t sp_canopy_workspace_bytes(int32_t dtype, int64_t n, int64_t d, int64_t chains, int64_t cap) {
  if ((dtype != SP_F32 && dtype != SP_F64) || !canopy_sizes_ok(n, d, chains, cap, d)) return 0;
  return sp_align256((size_t)chains * (size_t)cap * (size_t)d * sp_dtype_size(dtype));
}

extern "C" int sp_canopy(int32_t dtype, const void* d_X, int64_t ldx, int64_t n, int64_t d, double t1, double t2,
                         int64_t chains, int64_t cap, void* d_centers, int64_t ldc, int64_t* d_counts, int64_t* d_rows,
                         int64_t* d_num, void* d_ws, size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_canopy", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (!canopy_sizes_ok(n, d, chains, cap, ldc) || ldx < d)
      SP_FAIL("sp_canopy: bad shape n=%lld d=%lld ldx=%lld ldc=%lld chains=%lld cap=%lld (d, chains, cap >= 1; ldx, ldc >= d)",
              (long long)n, (long long)d, (long long)ldx, (long long)ldc, (long long)chains, (long long)cap);
    const T a1 = (T)t1, a2 = (T)t2;
    if (!std::isfinite(a1) || !std::isfinite(a2)) SP_FAIL("sp_canopy: t1 = %g and t2 = %g must be finite", t1, t2);
    if (!d_centers || !d_counts || !d_rows || !d_num || !d_ws || (n > 0 && !d_X))
      SP_FAIL("sp_canopy: X, centers, counts, rows, num and the workspace are required");
    if (ws_bytes < sp_canopy_workspace_bytes(dtype, n, d, chains, cap))
      SP_FAIL("sp_canopy: a workspace of %zu bytes, %zu needed", ws_bytes, sp_canopy_workspace_bytes(dtype, n, d, chains, cap));
    hipLaunchKernelGGL(canopy_kernel<T>, dim3((unsigned)chains), dim3(256), 0, (hipStream_t)stream, (const T*)d_X, ldx, n, d,
                       a1, a2, chains, cap, (T*)d_centers, ldc, d_counts, d_rows, d_num, (T*)d_ws);
    SP_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int sp_pdf_label(int32_t dtype, const void* d_X, int64_t ldx, int64_t n, const void* d_C, int64_t ldc, int64_t k,
                            int64_t d, int32_t* labels, void* stream) {
  return sp_float_dispatch("sp_pdf_label", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0 || k < 0 || k > 0x7fffffffLL || d < 1 || ldx < d || ldc < d || (n + 63) / 64 > 0x7fffffffLL)
      SP_FAIL("sp_pdf_label: bad shape n=%lld k=%lld d=%lld ldx=%lld ldc=%lld", (long long)n, (long long)k, (long long)d,
              (long long)ldx, (long long)ldc);
    if (n > 0 && (!d_X || !labels || (k > 0 && !d_C))) SP_FAIL("sp_pdf_label: X, C and labels are required");
    if (n == 0) return 0;
    hipLaunchKernelGGL(pdf_label_kernel<T>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)d_X, ldx, n, (const T*)d_C, ldc, k, d, labels);
    SP_CHECK_LAUNCH();
    return 0;
  });
}
