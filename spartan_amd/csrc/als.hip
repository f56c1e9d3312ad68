// One half-step of alternating least squares: per row of the ratings a weighted Gram accumulation and a small SPD
// solve, fused -- the tile body of the reference's
//   spartan/examples/als.py   _solve_U_or_M_mapper (:49-78: a Python loop over rows)
//                             _als_solver (:7-24), _implicit_feedback_als_solver (:27-46), both scipy.linalg.lstsq
// The contract is in include/spartan_hip_als.h.  Kernels:
//   als_rows_kernel<T, B>  a workgroup of 256 threads = 4 rows of R, one per wave.  The items pass through LDS 64 at a
//                          time: their rows of Y (shared by the four rows, zero-padded to fp = a multiple of B
//                          features; the next chunk is in flight in registers while this one is used) and each wave's
//                          64 ratings.  The lower triangle of A_i is cut into B x B blocks, T = nb (nb + 1) / 2 of them
//                          with nb = ceil(f / B); the wave is cut into G = floor(64 / T) groups of T lanes, a lane per
//                          block, and group g takes items g, g + G, g + 2 G, ... of every chunk: per item a lane reads
//                          2 B values of Y for B^2 FMAs (the lanes of diagonal blocks add b_i's B entries as well).
//                          B = 4 for f <= 32 (f <= 4 is a lane per item, f = 20 four items at a time), B = 8 above.
//                          Then the groups' accumulators are added in group order into the packed lower triangle in
//                          LDS (over the staging area), the diagonal terms are added and the wave factors and solves
//                          with lane p on row p.
//   als_gram_partial_kernel  implicit mode's Y^T Y: partial Grams over fixed ranges of items, then their sum in
//                          ascending order (sp_partial_sum_kernel, sp_extras_common.hpp; 0 for n = 0).
//   als_info_kernel        hands the lowest failing row of the call to *d_info if that is still 0.
// Vector pipe only; every sum is an explicit fma onto an accumulator that starts at 0.
#include <limits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_als.h"

namespace {

constexpr int ROWS = 4;        // rows of R per workgroup (one per wave)
constexpr int CH = 64;         // items per chunk
constexpr int SMALL_F = 32;    // f <= SMALL_F: 4 x 4 blocks; above: 8 x 8
constexpr int FLAG_BYTES = 256;           // head of the workspace: the word that collects the lowest failing row
constexpr int GRAM_RANGES = 1024;         // at most this many item ranges in the Y^T Y pre-pass

__host__ __device__ __forceinline__ int tri(int p) { return p * (p + 1) / 2; }

// the item ranges of the pre-pass: a multiple of CH long, at most GRAM_RANGES of them -- a function of n alone
int64_t gram_range_len(int64_t n) {
  int64_t len = (n + GRAM_RANGES - 1) / GRAM_RANGES;
  len = (len + CH - 1) / CH * CH;
  return len < 4 * CH ? 4 * CH : len;
}

// A chunk of CH rows of Y as [CH][pitch] in LDS, columns >= f and rows >= n zero.  Thread (ti, tc) of the 16 x 16 grid
// takes rows ti + 16 pass and columns tc + 16 c: 16 consecutive lanes read one 64- or 128-byte run.
template <typename T, int NC>
struct YChunk {
  T v[4][NC];
  __device__ __forceinline__ void fetch(const T* __restrict__ Y, int64_t ldy, int64_t n, int f, int64_t j0, int tid) {
    const int ti = tid >> 4, tc = tid & 15;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int64_t j = j0 + ti + 16 * pass;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = tc + 16 * c;
        v[pass][c] = (j < n && col < f) ? Y[j * ldy + col] : (T)0;
      }
    }
  }
  __device__ __forceinline__ void store(T* ys, int pitch, int tid) const {
    const int ti = tid >> 4, tc = tid & 15;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = tc + 16 * c;
        if (col < pitch) ys[(ti + 16 * pass) * pitch + col] = v[pass][c];
      }
  }
};

template <typename T, int B>
__global__ __launch_bounds__(256) void als_rows_kernel(const T* __restrict__ R, int64_t ldr, int64_t m, int64_t n,
                                                       const T* __restrict__ Y, int64_t ldy, int f, T la, T alpha,
                                                       int implicit, const T* __restrict__ gram, T* __restrict__ X,
                                                       int64_t ldx, int* __restrict__ lowest) {
  constexpr int NC = (B == 4 ? SMALL_F : SP_ALS_MAX_F) / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char als_smem[];
  const int nb = (f + B - 1) / B, fp = nb * B;
  T* ys = reinterpret_cast<T*>(als_smem);                  // [CH][fp]
  T* rs = ys + CH * fp;                                    // [ROWS][CH]
  // after the last chunk, over the same bytes:
  T* As = reinterpret_cast<T*>(als_smem);                  // [ROWS][tri(fp)]  packed lower triangles, row-major
  T* bs = As + ROWS * tri(fp);                             // [ROWS][fp]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = (int64_t)blockIdx.x * ROWS + wave;
  const bool have_row = row < m;

  // this lane's block of the triangle and its group of items
  const int nblk = tri(nb), G = 64 / nblk;
  const int g = lane / nblk, blk = lane - g * nblk;
  const bool worker = g < G;
  int bp = 0;
  while (tri(bp + 1) <= blk) ++bp;
  const int bq = blk - tri(bp);
  const bool diag = bp == bq;
  const int steps = (CH + G - 1) / G;

  T acc[B][B], bacc[B];
#pragma unroll
  for (int a = 0; a < B; ++a) {
    bacc[a] = (T)0;
#pragma unroll
    for (int b = 0; b < B; ++b) acc[a][b] = (T)0;
  }
  int64_t count = 0;                                       // |S_i| (wave-uniform)

  YChunk<T, NC> yn;
  T rn = (T)0;
  const int64_t nchunks = (n + CH - 1) / CH;
  auto fetch = [&](int64_t c) {
    yn.fetch(Y, ldy, n, f, c * CH, tid);
    const int64_t j = c * CH + lane;
    rn = (have_row && j < n) ? R[row * ldr + j] : (T)0;
  };
  if (nchunks > 0) fetch(0);
  for (int64_t c = 0; c < nchunks; ++c) {
    __syncthreads();                      // the previous chunk has been read by everyone
    yn.store(ys, fp, tid);
    rs[wave * CH + lane] = rn;
    const unsigned long long nz = __ballot(rn != (T)0);    // (true for NaN: it is counted, and fails the row below)
    count += __popcll(nz);
    __syncthreads();
    if (c + 1 < nchunks) fetch(c + 1);
    if (nz == 0) continue;                // (a wave's own branch: no workgroup barrier below)
    for (int s = 0; s < steps; ++s) {
      const int it = s * G + g;
      if (!worker || it >= CH) continue;
      const T r = rs[wave * CH + it];
      if (r != (T)0) {
        const T* yp = ys + it * fp + bp * B;
        const T* yq = ys + it * fp + bq * B;
        // B features of one item: 16-byte aligned in LDS (fp is a multiple of B >= 4)
        const VecN<T, B> lp = *reinterpret_cast<const VecN<T, B>*>(yp), lq = *reinterpret_cast<const VecN<T, B>*>(yq);
        const T* vp = lp.v;
        const T* vq = lq.v;
        const T w = implicit ? alpha * r : (T)1;
#pragma unroll
        for (int a = 0; a < B; ++a) {
          const T wy = w * vp[a];
#pragma unroll
          for (int b = 0; b < B; ++b) acc[a][b] = fma_t(wy, vq[b], acc[a][b]);
        }
        if (diag) {
          const T cw = implicit ? (r > (T)0 ? (T)1 + alpha * r : (T)0) : r;
#pragma unroll
          for (int a = 0; a < B; ++a) bacc[a] = fma_t(cw, vp[a], bacc[a]);
        }
      }
    }
  }
  __syncthreads();                        // staging is over: its bytes become the triangles

  // the groups' sums, added in group order
  T* Aw = As + wave * tri(fp);
  T* bw = bs + wave * fp;
  for (int g2 = 0; g2 < G; ++g2) {
    if (worker && g == g2) {
#pragma unroll
      for (int a = 0; a < B; ++a) {
        const int p = bp * B + a;
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const int q = bq * B + b;
          if (q <= p) Aw[tri(p) + q] = g2 == 0 ? acc[a][b] : Aw[tri(p) + q] + acc[a][b];
        }
        if (diag) bw[p] = g2 == 0 ? bacc[a] : bw[p] + bacc[a];
      }
    }
    sp_wave_sync();
  }
  if (!have_row) return;                  // (a whole wave; nothing below synchronises the workgroup)

  T* xrow = X + row * ldx;
  if (!implicit && count == 0) {          // nothing rated: the reference's lstsq of a zero system
    if (lane < f) xrow[lane] = (T)0;
    return;
  }
  if (implicit) {
    for (int p = 0; p < f; ++p)
      if (lane <= p) Aw[tri(p) + lane] = Aw[tri(p) + lane] + gram[p * f + lane];
    sp_wave_sync();
    if (lane < f) Aw[tri(lane) + lane] = Aw[tri(lane) + lane] + la;
  } else {
    const T ridge = la * (T)count;
    if (lane < f) Aw[tri(lane) + lane] = Aw[tri(lane) + lane] + ridge;
  }
  sp_wave_sync();

  // Cholesky, left-looking: lane p owns row p; column k of L needs columns 0 .. k - 1
  const int p = lane;
  const bool mine = p < f;
  bool bad = false;
  for (int k = 0; k < f; ++k) {
    T v = (T)0;
    if (mine && p >= k) {
      v = Aw[tri(p) + k];
      for (int q = 0; q < k; ++q) v = fma_t(-Aw[tri(p) + q], Aw[tri(k) + q], v);
    }
    const T d = __shfl(v, k);
    if (!(d > (T)0)) { bad = true; break; }                 // (wave-uniform; false for NaN)
    const T sd = sqrt_t(d);
    if (mine && p >= k) Aw[tri(p) + k] = p == k ? sd : v / sd;      // (column k: read by nobody in this step)
    sp_wave_sync();
  }
  T z = mine ? bw[p] : (T)0;
  if (__ballot(!(z - z == (T)0)) != 0) bad = true;           // b_i is not finite (a NaN rating in explicit mode)
  if (bad) {
    if (mine) xrow[p] = std::numeric_limits<T>::quiet_NaN();
    if (lane == 0) atomicMax(lowest, (int)(0x7fffffff - row));
    return;
  }
  for (int k = 0; k < f; ++k) {                             // L z = b
    const T zk = __shfl(z, k) / Aw[tri(k) + k];
    if (p == k) z = zk;
    else if (mine && p > k) z = fma_t(-Aw[tri(p) + k], zk, z);
  }
  for (int k = f - 1; k >= 0; --k) {                        // L^T x = z
    const T xk = __shfl(z, k) / Aw[tri(k) + k];
    if (p == k) z = xk;
    else if (p < k) z = fma_t(-Aw[tri(k) + p], xk, z);
  }
  if (mine) xrow[p] = z;
}

// partial[range][f * f] <- sum over the range's items of y_j y_j^T (the full square: both halves get the same bits)
template <typename T>
__global__ __launch_bounds__(256) void als_gram_partial_kernel(const T* __restrict__ Y, int64_t ldy, int64_t n, int f,
                                                               int64_t range_len, T* __restrict__ partial) {
  constexpr int NC = SP_ALS_MAX_F / 16, NE = SP_ALS_MAX_F * SP_ALS_MAX_F / 256;
  __shared__ T ys[CH * SP_ALS_MAX_F];
  const int tid = threadIdx.x;
  const int64_t j_begin = (int64_t)blockIdx.x * range_len;
  const int64_t j_end = j_begin + range_len < n ? j_begin + range_len : n;
  int ep[NE], eq[NE];
  T acc[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int e = tid + 256 * k;
    ep[k] = e < f * f ? e / f : -1;
    eq[k] = e < f * f ? e - ep[k] * f : 0;
    acc[k] = (T)0;
  }
  YChunk<T, NC> yn;
  for (int64_t j0 = j_begin; j0 < j_end; j0 += CH) {
    yn.fetch(Y, ldy, j_end, f, j0, tid);
    __syncthreads();
    yn.store(ys, f, tid);
    __syncthreads();
    const int jn = (int)(j_end - j0 < CH ? j_end - j0 : CH);
    for (int jj = 0; jj < jn; ++jj) {
#pragma unroll
      for (int k = 0; k < NE; ++k)
        if (ep[k] >= 0) acc[k] = fma_t(ys[jj * f + ep[k]], ys[jj * f + eq[k]], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < NE; ++k)
    if (ep[k] >= 0) partial[(int64_t)blockIdx.x * f * f + tid + 256 * k] = acc[k];
}

__global__ void als_info_kernel(const int* __restrict__ lowest, int* __restrict__ info) {
  const int v = *lowest;
  if (v != 0) atomicCAS(info, 0, 1 + (0x7fffffff - v));
}

size_t als_lds_bytes(int f, int B, size_t elem) {
  const int nb = (f + B - 1) / B, fp = nb * B;
  const size_t staging = (size_t)(CH * fp + ROWS * CH) * elem;
  const size_t solve = (size_t)(ROWS * tri(fp) + ROWS * fp) * elem;
  return staging > solve ? staging : solve;
}

template <typename T>
int als_run(const T* R, int64_t ldr, int64_t m, int64_t n, const T* Y, int64_t ldy, int32_t f, double la, double alpha,
            int32_t implicit, T* X, int64_t ldx, int32_t* info, void* ws, hipStream_t st) {
  int* lowest = reinterpret_cast<int*>(ws);
  SP_HIP(hipMemsetAsync(lowest, 0, sizeof(int), st));
  T* gram = nullptr;
  if (implicit) {
    gram = reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(ws) + FLAG_BYTES);
    T* partial = reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(gram) + sp_align256((size_t)f * f * sizeof(T)));
    const int64_t len = gram_range_len(n), ranges = (n + len - 1) / len;
    if (ranges > 0) {
      hipLaunchKernelGGL(als_gram_partial_kernel<T>, dim3((unsigned)ranges), dim3(256), 0, st, Y, ldy, n, (int)f, len,
                         partial);
      SP_CHECK_LAUNCH();
    }
    if (sp_partial_sum<T>(partial, ranges, f, f, gram, f, (const T*)nullptr, 0, (T*)nullptr, st)) return 1;
  }
  const unsigned blocks = (unsigned)((m + ROWS - 1) / ROWS);
  if (f <= SMALL_F) {
    const size_t lds = als_lds_bytes(f, 4, sizeof(T));
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(als_rows_kernel<T, 4>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((als_rows_kernel<T, 4>), dim3(blocks), dim3(256), lds, st, R, ldr, m, n, Y, ldy, (int)f, (T)la,
                       (T)alpha, (int)implicit, gram, X, ldx, lowest);
  } else {
    const size_t lds = als_lds_bytes(f, 8, sizeof(T));
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(als_rows_kernel<T, 8>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((als_rows_kernel<T, 8>), dim3(blocks), dim3(256), lds, st, R, ldr, m, n, Y, ldy, (int)f, (T)la,
                       (T)alpha, (int)implicit, gram, X, ldx, lowest);
  }
  SP_CHECK_LAUNCH();
  hipLaunchKernelGGL(als_info_kernel, dim3(1), dim3(1), 0, st, lowest, info);
  SP_CHECK_LAUNCH();
  return 0;
}

bool als_args_ok(int32_t dtype, int64_t m, int64_t n, int32_t f) {
  return (dtype == SP_F32 || dtype == SP_F64) && m >= 0 && n >= 0 && f >= 1 && f <= SP_ALS_MAX_F;
}

}  // namespace

extern "C" size_t sp_als_solve_workspace_bytes(int32_t dtype, int64_t m, int64_t n, int32_t f, int32_t implicit) {
  (void)m;
  if (!als_args_ok(dtype, m, n, f)) return 0;
  if (!implicit) return FLAG_BYTES;
  const int64_t len = gram_range_len(n), ranges = (n + len - 1) / len;
  const size_t sq = sp_align256((size_t)f * f * sp_dtype_size(dtype));
  return FLAG_BYTES + sq + (size_t)(ranges > 0 ? ranges : 1) * sq;
}

extern "C" int sp_als_solve(int32_t dtype, const void* d_R, int64_t ldr, int64_t m, int64_t n, const void* d_Y,
                            int64_t ldy, int32_t f, double la, double alpha, int32_t implicit, void* d_X, int64_t ldx,
                            int32_t* d_info, void* d_ws, size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_als_solve", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (f < 1 || f > SP_ALS_MAX_F) SP_FAIL("sp_als_solve: f = %d is outside 1 .. %d", (int)f, SP_ALS_MAX_F);
    if (m < 0 || n < 0 || ldr < n || ldy < f || ldx < f)
      SP_FAIL("sp_als_solve: bad shape m=%lld n=%lld f=%d ldr=%lld ldy=%lld ldx=%lld", (long long)m, (long long)n, (int)f,
              (long long)ldr, (long long)ldy, (long long)ldx);
    if (m > 0x7ffffffeLL) SP_FAIL("sp_als_solve: %lld rows in one call (at most 2^31 - 2)", (long long)m);
    if (m == 0) return 0;
    const size_t need = sp_als_solve_workspace_bytes(dtype, m, n, f, implicit);
    if (!d_info || !d_ws || ws_bytes < need) SP_FAIL("sp_als_solve: info word or workspace missing (%zu bytes, %zu needed)",
                                                     ws_bytes, need);
    return als_run<T>((const T*)d_R, ldr, m, n, (const T*)d_Y, ldy, f, la, alpha, implicit, (T*)d_X, ldx, d_info, d_ws,
                      (hipStream_t)stream);
  });
}
