// One iteration of the reference's fuzzy k-means on a row tile, memberships and weighted sums fused:
//   spartan/examples/fuzzy_kmeans.py   kmeans_map2_dist_mapper   (:41-50: cdist, ** 1 / (m - 1), row-normalise)
//                                      kmeans_map2_center_mapper (:53-62: dot(X.T, fuzzy ** m))
// The contract is in include/spartan_hip_fuzzy.h.  Three kernels:
//   fuzzy_norm_kernel        a workgroup of 256 threads = 64 rows x all centres.  The distance tile is the one sp_knn
//                            uses (sp_d2_tile, sp_extras_common.hpp): centres pass through LDS 64 at a time, both
//                            operands in chunks of 16 features stored feature-major with a row pitch of 68, the next
//                            chunk in flight in registers; thread (ty, tx) of the 16 x 16 grid holds the 4 x 4 values of
//                            d2 of rows 4 ty .. 4 ty + 3 and centres 4 tx .. 4 tx + 3, each ONE accumulator.  The 16
//                            lanes that share a row are neighbours in a wave: the row's arg-max of d2 and its sum of p
//                            are butterflies over those lanes (the order is in the header), no LDS and no barrier.
//   fuzzy_accumulate_kernel  a workgroup = 64 centres x a panel of 128 features x a range of row blocks.  Per block of
//                            64 rows: the same distance tile, w = (p / z)^m into LDS [row][centre], the rows' panel of
//                            X into LDS [row][feature], then 64 steps r = 0 .. 63 in which thread (tf, tc) adds
//                            w[r][4 tc ..] x[r][8 tf ..] onto its 4 x 8 sums (two aligned 16-byte reads of w and x for
//                            32 multiply-adds); the threads of tf = 0 carry wsum of their centres.
//   sp_partial_sum_kernel    the ranges' partials, added in ascending order: the k x d sums and the k weights behind
//                            them in one launch (sp_extras_common.hpp).
#include <cmath>
#include <limits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_fuzzy.h"

namespace {

constexpr int RB = SP_FUZZY_ROWS;      // rows per workgroup
constexpr int CB = SP_FUZZY_CENTERS;   // centres per pass
constexpr int FP = SP_FUZZY_PANEL;     // features per panel of the accumulation
constexpr int DC = SP_D2_DC;           // features per chunk of the distance tile
constexpr int PITCH = SP_D2_PITCH;     // elements between the feature rows of a staged chunk
constexpr int WP = CB + 4;             // elements between the rows of the staged weights
constexpr int XP = FP + 4;             // elements between the rows of the staged panel
static_assert(RB == 64 && CB == 64 && FP == 128, "the thread maps below are written for 64 x 64 x 128");

// the scalars of a call, each rounded to T once on the host
template <typename T>
struct Scalars {
  T e;        // 1 / (m - 1)
  T m;
  T tiny;     // 1e-10
  int m2;     // m == 2 exactly: no pow
};

template <typename T>
__device__ __forceinline__ T fz_p(T d2, const Scalars<T>& s) {
  T dist = sqrt_t(d2);
  if (dist == (T)0) dist = s.tiny;
  return s.m2 ? dist : pow_t(dist, s.e);
}

template <typename T>
__device__ __forceinline__ T fz_w(T u, const Scalars<T>& s) {
  return s.m2 ? u * u : pow_t(u, s.m);
}

// (a, ia) comes before (b, ib) in the order of the arg-max: a NaN above every number, then the larger value, then the
// lower index.  A total order on distinct indices, so a reduction finds the same winner in any order.
template <typename T>
__device__ __forceinline__ bool beats(T a, int64_t ia, T b, int64_t ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}

template <typename T>
__global__ __launch_bounds__(256) void fuzzy_norm_kernel(const T* __restrict__ X, int64_t ldx, int64_t n,
                                                         const T* __restrict__ C, int64_t ldc, int64_t k, int64_t d,
                                                         Scalars<T> sc, int64_t* __restrict__ labels,
                                                         T* __restrict__ z_out, T* __restrict__ U, int64_t ldu) {
  __shared__ __attribute__((aligned(16))) T xs[DC * PITCH];
  __shared__ __attribute__((aligned(16))) T cs[DC * PITCH];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t r0 = (int64_t)blockIdx.x * RB;

  T z[4], bv[4];
  int64_t bi[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    z[a] = (T)0;
    bv[a] = (T)-1;                      // (below every d2: centre 0 always replaces it)
    bi[a] = 0;
  }

  T acc[4][4];
  for (int64_t c0 = 0; c0 < k; c0 += CB) {
    sp_d2_tile<T>(X, ldx, n, r0, C, ldc, k, c0, d, xs, cs, tid, acc);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      T g = (T)0, v = (T)-1;
      int64_t vi = std::numeric_limits<int64_t>::max();
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t c = c0 + tx * 4 + b;
        const bool valid = c < k;
        const T p = valid ? fz_p(acc[a][b], sc) : (T)0;
        g = g + p;
        if (valid && beats(acc[a][b], c, v, vi)) {
          v = acc[a][b];
          vi = c;
        }
      }
      // the 16 lanes tx = 0 .. 15 of this row: a balanced tree (addition commutes, so every lane holds the same bits)
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) {
        g = g + __shfl_xor(g, s);
        const T ov = __shfl_xor(v, s);
        const int64_t oi = __shfl_xor(vi, s);
        if (beats(ov, oi, v, vi)) {
          v = ov;
          vi = oi;
        }
      }
      z[a] = z[a] + g;
      if (beats(v, vi, bv[a], bi[a])) {
        bv[a] = v;
        bi[a] = vi;
      }
    }
  }

  if (tx == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t row = r0 + ty * 4 + a;
      if (row < n) {
        if (labels) labels[row] = bi[a];
        z_out[row] = z[a];
      }
    }
  }

  if (U) {
    for (int64_t c0 = 0; c0 < k; c0 += CB) {
      sp_d2_tile<T>(X, ldx, n, r0, C, ldc, k, c0, d, xs, cs, tid, acc);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int64_t row = r0 + ty * 4 + a;
        if (row >= n) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int64_t c = c0 + tx * 4 + b;
          if (c < k) U[row * ldu + c] = fz_p(acc[a][b], sc) / z[a];
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fuzzy_accumulate_kernel(const T* __restrict__ X, int64_t ldx, int64_t n,
                                                               const T* __restrict__ C, int64_t ldc, int64_t k,
                                                               int64_t d, Scalars<T> sc, const T* __restrict__ zin,
                                                               int64_t cblocks, int64_t panels, int64_t ranges,
                                                               T* __restrict__ S, int64_t lds, int64_t s_stride,
                                                               T* __restrict__ W, int64_t w_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fuzzy_smem[];
  T* xs = reinterpret_cast<T*>(fuzzy_smem);      // [DC][PITCH]
  T* cs = xs + DC * PITCH;                       // [DC][PITCH]
  T* wt = cs + DC * PITCH;                       // [RB][WP]
  T* xp = wt + RB * WP;                          // [RB][XP]

  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int tc = tid & 15, tf = tid >> 4;
  const int64_t bid = blockIdx.x;
  const int64_t cbk = bid % cblocks, pn = (bid / cblocks) % panels, g = bid / (cblocks * panels);
  const int64_t c0 = cbk * CB, f0 = pn * FP;
  const int64_t nb = (n + RB - 1) / RB;
  const int64_t rb_b = g * nb / ranges, rb_e = (g + 1) * nb / ranges;

  T sacc[4][8], wacc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    wacc[a] = (T)0;
#pragma unroll
    for (int j = 0; j < 8; ++j) sacc[a][j] = (T)0;
  }

  T acc[4][4];
  for (int64_t rb = rb_b; rb < rb_e; ++rb) {
    const int64_t r0 = rb * RB;
    sp_d2_tile<T>(X, ldx, n, r0, C, ldc, k, c0, d, xs, cs, tid, acc);
    __syncthreads();                    // the previous block's weights and panel have been read by everyone
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t row = r0 + ty * 4 + a;
      const bool rv = row < n;
      const T zr = rv ? zin[row] : (T)1;
      Vec4<T> wv;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t c = c0 + tx * 4 + b;
        wv.v[b] = (rv && c < k) ? fz_w(fz_p(acc[a][b], sc) / zr, sc) : (T)0;
      }
      *reinterpret_cast<Vec4<T>*>(wt + (ty * 4 + a) * WP + tx * 4) = wv;
    }
#pragma unroll 4
    for (int i = 0; i < RB * FP / 256; ++i) {
      const int idx = i * 256 + tid;
      const int r = idx / FP, f = idx % FP;
      const int64_t row = r0 + r, col = f0 + f;
      xp[r * XP + f] = (row < n && col < d) ? X[row * ldx + col] : (T)0;
    }
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < RB; ++r) {
      const Vec4<T> wv = *reinterpret_cast<const Vec4<T>*>(wt + r * WP + tc * 4);
      const Vec4<T> x0 = *reinterpret_cast<const Vec4<T>*>(xp + r * XP + tf * 8);
      const Vec4<T> x1 = *reinterpret_cast<const Vec4<T>*>(xp + r * XP + tf * 8 + 4);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sacc[a][j] = sacc[a][j] + wv.v[a] * x0.v[j];
          sacc[a][j + 4] = sacc[a][j + 4] + wv.v[a] * x1.v[j];
        }
        if (tf == 0) wacc[a] = wacc[a] + wv.v[a];
      }
    }
  }

  T* So = S + g * s_stride;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int64_t c = c0 + tc * 4 + a;
    if (c >= k) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t col = f0 + tf * 8 + j;
      if (col < d) So[c * lds + col] = sacc[a][j];
    }
    if (pn == 0 && tf == 0) W[g * w_stride + c] = wacc[a];
  }
}

int64_t fz_cblocks(int64_t k) { return (k + CB - 1) / CB; }
int64_t fz_panels(int64_t d) { return d > 0 ? (d + FP - 1) / FP : 1; }      // (d = 0: one panel, for wsum)

// the number of ranges the row blocks are cut into
int64_t fz_ranges(int64_t n, int64_t k, int64_t d, int32_t splits) {
  const int64_t nb = (n + RB - 1) / RB;
  if (nb <= 1) return 1;
  if (splits >= 1) return splits < nb ? splits : nb;
  // the library's choice: about two workgroups per CU, every range at least eight row blocks long so that the
  // partials (ranges x k x d) stay small beside the rows read
  const int64_t per = fz_cblocks(k) * fz_panels(d);
  int64_t want = (2 * SP_CUS + per - 1) / per;
  if (want > nb / 8) want = nb / 8;
  if (want > 64) want = 64;
  return want < 1 ? 1 : want;
}

// the workspace: z (a value per row), then with more than one range their partial sums and partial weights
struct Layout {
  int64_t ranges;
  size_t z_bytes, s_bytes, w_bytes;
  size_t total() const { return z_bytes + s_bytes + w_bytes; }
};

Layout fz_layout(size_t sz, int64_t n, int64_t k, int64_t d, int32_t splits) {
  Layout l;
  l.ranges = fz_ranges(n, k, d, splits);
  l.z_bytes = sp_align256((size_t)(n > 0 ? n : 1) * sz);
  l.s_bytes = l.ranges > 1 ? sp_align256((size_t)l.ranges * k * d * sz) : 0;
  l.w_bytes = l.ranges > 1 ? (size_t)l.ranges * k * sz : 0;
  return l;
}

template <typename T>
int fz_run(const T* X, int64_t ldx, int64_t n, const T* C, int64_t ldc, int64_t k, int64_t d, double m, int32_t splits,
           int64_t* labels, T* S, int64_t lds, T* W, T* U, int64_t ldu, void* ws, size_t ws_bytes, hipStream_t st) {
  const Layout l = fz_layout(sizeof(T), n, k, d, splits);
  const int64_t ranges = l.ranges, cblocks = fz_cblocks(k), panels = fz_panels(d), nb = (n + RB - 1) / RB;
  if (!ws || ws_bytes < l.total()) SP_FAIL("sp_fuzzy_step: workspace of %zu bytes, %zu needed", ws_bytes, l.total());
  if (nb > 0x7fffffffLL || (double)cblocks * (double)panels * (double)ranges > 2147483647.0)
    SP_FAIL("sp_fuzzy_step: n=%lld k=%lld d=%lld are too many workgroups for one launch", (long long)n, (long long)k,
            (long long)d);
  unsigned char* wsb = reinterpret_cast<unsigned char*>(ws);
  T* z = reinterpret_cast<T*>(wsb);
  T* ps = reinterpret_cast<T*>(wsb + l.z_bytes);
  T* pw = reinterpret_cast<T*>(wsb + l.z_bytes + l.s_bytes);

  Scalars<T> sc;
  sc.e = (T)(1.0 / (m - 1.0));
  sc.m = (T)m;
  sc.tiny = (T)1e-10;
  sc.m2 = m == 2.0;

  if (n > 0) {
    hipLaunchKernelGGL(fuzzy_norm_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, X, ldx, n, C, ldc, k, d, sc, labels, z,
                       U, ldu);
    SP_CHECK_LAUNCH();
  }
  const size_t smem = (size_t)(2 * DC * PITCH + RB * WP + RB * XP) * sizeof(T);
  SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fuzzy_accumulate_kernel<T>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  if (ranges > 1)
    hipLaunchKernelGGL(fuzzy_accumulate_kernel<T>, dim3((unsigned)(cblocks * panels * ranges)), dim3(256), smem, st, X,
                       ldx, n, C, ldc, k, d, sc, z, cblocks, panels, ranges, ps, d, k * d, pw, k);
  else
    hipLaunchKernelGGL(fuzzy_accumulate_kernel<T>, dim3((unsigned)(cblocks * panels)), dim3(256), smem, st, X, ldx, n, C,
                       ldc, k, d, sc, z, cblocks, panels, (int64_t)1, S, lds, (int64_t)0, W, (int64_t)0);
  SP_CHECK_LAUNCH();
  // S[j, f] <- P_0[j, f] + P_1[j, f] + ... in ascending order; the same for the k weights behind the k * d sums
  if (ranges > 1) return sp_partial_sum<T>(ps, ranges, k, d, S, lds, pw, k, W, st);
  return 0;
}

bool fz_shape_ok(int64_t n, int64_t k, int64_t d, int32_t splits) { return n >= 0 && k >= 1 && d >= 0 && splits >= 0; }

}  // namespace

extern "C" size_t sp_fuzzy_step_workspace_bytes(int32_t dtype, int64_t n, int64_t k, int64_t d, int32_t splits) {
  if ((dtype != SP_F32 && dtype != SP_F64) || !fz_shape_ok(n, k, d, splits)) return 0;
  return fz_layout(sp_dtype_size(dtype), n, k, d, splits).total();
}

extern "C" int sp_fuzzy_step(int32_t dtype, const void* d_X, int64_t ldx, int64_t n, const void* d_C, int64_t ldc,
                             int64_t k, int64_t d, double m, int32_t splits, int64_t* d_labels, void* d_sums,
                             int64_t lds, void* d_wsum, void* d_U, int64_t ldu, void* d_ws, size_t ws_bytes,
                             void* stream) {
  return sp_float_dispatch("sp_fuzzy_step", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (!(m > 1.0) || std::isinf(m)) SP_FAIL("sp_fuzzy_step: m = %g must be finite and > 1", m);
    if (k < 1) SP_FAIL("sp_fuzzy_step: k = %lld must be at least 1", (long long)k);
    if (!fz_shape_ok(n, k, d, splits) || ldx < d || ldc < d || lds < d || (d_U && ldu < k))
      SP_FAIL("sp_fuzzy_step: bad shape n=%lld k=%lld d=%lld ldx=%lld ldc=%lld lds=%lld ldu=%lld splits=%d", (long long)n,
              (long long)k, (long long)d, (long long)ldx, (long long)ldc, (long long)lds, (long long)ldu, (int)splits);
    if (!d_wsum || (!d_sums && d > 0)) SP_FAIL("sp_fuzzy_step: sums and wsum are required");
    if (n > 0 && d > 0 && (!d_X || !d_C)) SP_FAIL("sp_fuzzy_step: X and C are required");
    return fz_run<T>((const T*)d_X, ldx, n, (const T*)d_C, ldc, k, d, m, splits, d_labels, (T*)d_sums, lds, (T*)d_wsum,
                     (T*)d_U, ldu, d_ws, ws_bytes, (hipStream_t)stream);
  });
}
