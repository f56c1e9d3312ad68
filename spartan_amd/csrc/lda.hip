// One CVB0 step of the reference's LDA on a tile of documents, the per-document loops fused into two small matrix
// products around a quotient:
//   spartan/examples/lda.py   _lda_train (:7-52), _lda_mapper (:56-80), _lda_doc_topic_mapper (:84-110)
// The contract is in include/spartan_hip_lda.h.  With A[t, j] = (N[t, j] + eta) / (ts[t] + eta V), B[d, t] =
// gamma[d, t] + alpha, S = A^T B^T (V x D) and W = X / S where X != 0:  c = B o (|W|^T |A|^T),  delta = A o (B^T W^T).
// Four kernels:
//   lda_prep_kernel     a workgroup per topic: ts in a fixed order, then A to the workspace as [V][KP] (the topics of a
//                       term contiguous, KP = k rounded up to 16, 32, 64 or 128, the padding 0).
//   lda_gamma_kernel    a workgroup of 256 threads = 64 documents, B topic-major in LDS.  Per inner iteration the terms
//                       pass in chunks: X chunk [term][doc] and A chunk [topic][term] into LDS, thread (ty, tx) of the
//                       16 x 16 grid forms the S values of RA terms x 4 documents (inner dimension KP), overwrites its
//                       own x by |x / s|, then thread (cy, cx) adds |a| |w| onto c of documents 4 cx .. 4 cx + 3 and
//                       topics cy, cy + 16, ..: KT + 4 reads of 4 elements for 16 KT multiply-adds.  The next chunk is
//                       in flight in registers meanwhile.
//   lda_delta_kernel    a workgroup = 64 terms x a range of document blocks, its A block topic-major in LDS; per
//                       sub-block of documents the stored B and X into LDS, the S tile, the signed quotient, and
//                       acc[term][topic] += w b over the documents, a thread 4 terms x KT topics.
//   sp_partial_sum_kernel  the ranges' partials, added in ascending order (also the zero fill of D = 0;
//                       sp_extras_common.hpp).
#include <cmath>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_lda.h"

namespace {

constexpr int DB = SP_LDA_DOCS;        // documents per workgroup of lda_gamma_kernel, and the unit of `splits`
constexpr int TB = SP_LDA_TERMS;       // terms per workgroup of lda_delta_kernel
constexpr int PD = DB + 4;             // elements between LDS rows that hold 64 values
static_assert(DB == 64 && TB == 64, "the thread maps below are written for 64 x 64");

// what the LDS budget decides (the arithmetic is in the header): terms per chunk of lda_gamma_kernel and documents per
// sub-block of lda_delta_kernel -- 64, but 32 in fp64 and with 8 topics per thread (KP = 128), where 64 would need
// more than the 160 KB of a compute unit (fp64) or leave room for one workgroup per compute unit only (fp32)
template <typename T, int KT>
struct Cfg {
  static constexpr int TC = (sizeof(T) == 8 || KT == 8) ? 32 : 64;
  static constexpr int DC = TC;
};

// s[a][b] <- sum_t As[t][RA ty + a] Bs[t][RB tx + b], t = 0 .. kp - 1 ascending onto one accumulator that starts at 0
template <typename T, int RA, int RB>
__device__ __forceinline__ void s_tile(const T* as, int pa, const T* bs, int pb, int kp, int ty, int tx, T (&s)[RA][RB]) {
#pragma unroll
  for (int a = 0; a < RA; ++a)
#pragma unroll
    for (int b = 0; b < RB; ++b) s[a][b] = (T)0;
#pragma unroll 4
  for (int t = 0; t < kp; ++t) {
    const VecN<T, RA> av = *reinterpret_cast<const VecN<T, RA>*>(as + t * pa + ty * RA);
    const VecN<T, RB> bv = *reinterpret_cast<const VecN<T, RB>*>(bs + t * pb + tx * RB);
#pragma unroll
    for (int a = 0; a < RA; ++a)
#pragma unroll
      for (int b = 0; b < RB; ++b) s[a][b] = s[a][b] + av.v[a] * bv.v[b];
  }
}

// ts_t = sum_j |N_tj|: thread i adds j = i, i + 256, .. in ascending order onto 0, the 256 partial sums are added as a
// binary tree (i with i + 128, then + 64, .. + 1).  A[j][t] = (N_tj + eta) / (ts_t + eta V); topics k .. KP - 1 get 0.
template <typename T>
__global__ __launch_bounds__(256) void lda_prep_kernel(const T* __restrict__ N, int64_t ldn, int64_t V, int64_t k,
                                                       int kp, T eta, T* __restrict__ A) {
  __shared__ T red[256];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= k) {
    for (int64_t j = tid; j < V; j += 256) A[j * kp + t] = (T)0;
    return;
  }
  T part = (T)0;
  for (int64_t j = tid; j < V; j += 256) part = part + abs_t(N[t * ldn + j]);
  red[tid] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const T den = red[0] + eta * (T)V;
  for (int64_t j = tid; j < V; j += 256) A[j * kp + t] = (N[t * ldn + j] + eta) / den;
}

template <typename T, int KT>
__global__ __launch_bounds__(256) void lda_gamma_kernel(const T* __restrict__ X, int64_t ldx, int64_t V, int64_t D,
                                                        const T* __restrict__ A, int64_t k, T alpha, int iters,
                                                        T* __restrict__ Bst, T* __restrict__ doc_topics, int64_t ldt) {
  constexpr int KP = 16 * KT, TC = Cfg<T, KT>::TC, RA = TC / 16, PA = TC + 4;
  constexpr int NX = TC * DB / 256, NA = TC * KP / 256;      // elements of a chunk of X and of A per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char lda_smem[];
  T* bs = reinterpret_cast<T*>(lda_smem);        // [KP][PD]   B, topic-major
  T* as = bs + KP * PD;                          // [KP][PA]   the chunk of A, topic-major
  T* ws = as + KP * PA;                          // [TC][PD]   the chunk of X, then of |W|, term-major
  T* sums = ws + TC * PD;                        // [DB]
  int* nz = reinterpret_cast<int*>(sums + DB);   // [DB]       the document has a non-zero term

  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, cy = ty, cx = tx;
  const int64_t d0 = (int64_t)blockIdx.x * DB;
  const T g0 = (T)1 / (T)k;

  for (int idx = tid; idx < KP * DB; idx += 256) {
    const int t = idx >> 6, dd = idx & 63;
    bs[t * PD + dd] = t < k ? g0 + alpha : (T)0;
  }
  if (tid < DB) nz[tid] = 0;

  for (int it = 0; it < iters; ++it) {
    T c[4][KT];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int i = 0; i < KT; ++i) c[b][i] = (T)0;

    // the next chunk of X and A is in flight in registers while this one is worked on
    T xr[NX], ar[NA];
    auto fetch = [&](int64_t j0) {
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int idx = tid + 256 * i, jj = idx >> 6, dd = idx & 63;
        const int64_t j = j0 + jj, d = d0 + dd;
        xr[i] = (j < V && d < D) ? X[j * ldx + d] : (T)0;
      }
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int idx = tid + 256 * i, jj = idx / KP, t = idx % KP;
        ar[i] = (j0 + jj < V) ? A[(j0 + jj) * KP + t] : (T)0;
      }
    };
    if (V > 0) fetch(0);
    for (int64_t j0 = 0; j0 < V; j0 += TC) {
      __syncthreads();                  // the previous chunk has been read by everyone; B is in place
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int idx = tid + 256 * i;
        ws[(idx >> 6) * PD + (idx & 63)] = xr[i];
      }
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int idx = tid + 256 * i;
        as[(idx % KP) * PA + idx / KP] = ar[i];
      }
      __syncthreads();
      if (j0 + TC < V) fetch(j0 + TC);
      T s[RA][4];
      s_tile<T, RA, 4>(as, PA, bs, PD, KP, ty, tx, s);
#pragma unroll
      for (int a = 0; a < RA; ++a) {
        T* wp = ws + (ty * RA + a) * PD + tx * 4;
        VecN<T, 4> xv = *reinterpret_cast<const VecN<T, 4>*>(wp);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const T x = xv.v[b];
          if (x != (T)0) nz[tx * 4 + b] = 1;
          xv.v[b] = x != (T)0 ? abs_t(x / s[a][b]) : (T)0;      // (a pair with x = 0 is skipped: no quotient is formed)
        }
        *reinterpret_cast<VecN<T, 4>*>(wp) = xv;
      }
      __syncthreads();
      // c[d][t] += |a_tj| |w_jd|, j ascending
#pragma unroll 2
      for (int jj = 0; jj < TC; jj += 4) {
        VecN<T, 4> wv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wv[q] = *reinterpret_cast<const VecN<T, 4>*>(ws + (jj + q) * PD + cx * 4);
#pragma unroll
        for (int i = 0; i < KT; ++i) {
          const VecN<T, 4> av = *reinterpret_cast<const VecN<T, 4>*>(as + (cy + 16 * i) * PA + jj);
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int b = 0; b < 4; ++b) c[b][i] = c[b][i] + abs_t(av.v[q]) * wv[q].v[b];
        }
      }
    }
    __syncthreads();                    // every sweep is finished: B and nz are final for this iteration

    const bool last = it == iters - 1;
    if (last && Bst) {
      // the B that entered the last iteration, for lda_delta_kernel; 0 for an empty document, whose pairs then add
      // w b = 0 . 0 and never 0 . NaN
      for (int idx = tid; idx < DB * KP; idx += 256) {
        const int dd = idx / KP, t = idx % KP;
        if (d0 + dd < D) Bst[(d0 + dd) * KP + t] = nz[dd] ? bs[t * PD + dd] : (T)0;
      }
      __syncthreads();
    }
    // c_t = b_t . sum_j |a_tj| |w_j|, in place of b (a thread touches its own 4 x KT elements only)
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      const int t = cy + 16 * i;
      if (t < k) {
#pragma unroll
        for (int b = 0; b < 4; ++b) bs[t * PD + cx * 4 + b] = bs[t * PD + cx * 4 + b] * c[b][i];
      }
    }
    __syncthreads();
    if (tid < DB) {                     // sum_t c_t, t ascending onto 0
      T z = (T)0;
      for (int t = 0; t < k; ++t) z = z + bs[t * PD + tid];
      sums[tid] = z;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      const int t = cy + 16 * i;
      if (t < k) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int dd = cx * 4 + b;
          const T g = bs[t * PD + dd] / sums[dd];
          if (last) {
            if (doc_topics && d0 + dd < D) doc_topics[(d0 + dd) * ldt + t] = g;
          } else {
            bs[t * PD + dd] = g + alpha;
          }
        }
      }
    }
  }
}

template <typename T, int KT>
__global__ __launch_bounds__(256) void lda_delta_kernel(const T* __restrict__ X, int64_t ldx, int64_t V, int64_t D,
                                                        const T* __restrict__ A, int64_t k, const T* __restrict__ Bst,
                                                        int64_t tblocks, int64_t ranges, T* __restrict__ out,
                                                        int64_t ldo, int64_t out_stride) {
  constexpr int KP = 16 * KT, DC = Cfg<T, KT>::DC, RB = DC / 16, PB = DC + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char lda_smem[];
  T* as = reinterpret_cast<T*>(lda_smem);        // [KP][PD]   this workgroup's block of A, topic-major
  T* bs = as + KP * PD;                          // [KP][PB]   the sub-block of the stored B, topic-major
  T* ws = bs + KP * PB;                          // [TB][PB]   the sub-block of X, then of W, term-major

  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, cy = ty, cx = tx;
  const int64_t tb = (int64_t)blockIdx.x % tblocks, g = (int64_t)blockIdx.x / tblocks;
  const int64_t j0 = tb * TB;
  const int64_t nb = (D + DB - 1) / DB;
  const int64_t db_b = g * nb / ranges, db_e = (g + 1) * nb / ranges;
  const int64_t d_end = db_e * DB < D ? db_e * DB : D;

  for (int idx = tid; idx < TB * KP; idx += 256) {
    const int jj = idx / KP, t = idx % KP;
    as[t * PD + jj] = (j0 + jj < V) ? A[(j0 + jj) * KP + t] : (T)0;
  }

  T acc[4][KT];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < KT; ++i) acc[a][i] = (T)0;

  // the next sub-block of X and of the stored B is in flight in registers while this one is worked on
  constexpr int NX = TB * DC / 256, NB = DC * KP / 256;
  T xr[NX], br[NB];
  auto fetch = [&](int64_t d0) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int idx = tid + 256 * i, jj = idx / DC, dd = idx % DC;
      const int64_t j = j0 + jj, d = d0 + dd;
      xr[i] = (j < V && d < D) ? X[j * ldx + d] : (T)0;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + 256 * i, dd = idx / KP, t = idx % KP;
      br[i] = (d0 + dd < D) ? Bst[(d0 + dd) * KP + t] : (T)0;
    }
  };
  if (db_b * DB < d_end) fetch(db_b * DB);
  for (int64_t d0 = db_b * DB; d0 < d_end; d0 += DC) {
    __syncthreads();                    // the previous sub-block has been read by everyone; A is in place
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int idx = tid + 256 * i;
      ws[(idx / DC) * PB + idx % DC] = xr[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + 256 * i;
      bs[(idx % KP) * PB + idx / KP] = br[i];
    }
    __syncthreads();
    if (d0 + DC < d_end) fetch(d0 + DC);
    T s[4][RB];
    s_tile<T, 4, RB>(as, PD, bs, PB, KP, ty, tx, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      T* wp = ws + (ty * 4 + a) * PB + tx * RB;
      VecN<T, RB> xv = *reinterpret_cast<const VecN<T, RB>*>(wp);
#pragma unroll
      for (int b = 0; b < RB; ++b) {
        const T x = xv.v[b];
        xv.v[b] = x != (T)0 ? x / s[a][b] : (T)0;
      }
      *reinterpret_cast<VecN<T, RB>*>(wp) = xv;
    }
    __syncthreads();
    // acc[j][t] += w_jd b_dt, d ascending
#pragma unroll 2
    for (int dd = 0; dd < DC; dd += 4) {
      VecN<T, 4> wv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) wv[a] = *reinterpret_cast<const VecN<T, 4>*>(ws + (cx + 16 * a) * PB + dd);
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        const VecN<T, 4> bv = *reinterpret_cast<const VecN<T, 4>*>(bs + (cy + 16 * i) * PB + dd);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int a = 0; a < 4; ++a) acc[a][i] = acc[a][i] + wv[a].v[q] * bv.v[q];
      }
    }
  }
  __syncthreads();                      // (A is in place even if the loop above did not run)

  T* o = out + g * out_stride;
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int t = cy + 16 * i;
    if (t >= k) continue;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int jj = cx + 16 * a;
      if (j0 + jj < V) o[t * ldo + j0 + jj] = as[t * PD + jj] * acc[a][i];
    }
  }
}

int lda_kt(int64_t k) { return k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : 8; }

// the number of ranges the document blocks are cut into
int64_t lda_ranges(int64_t V, int64_t D, int64_t k, int32_t splits) {
  const int64_t nb = (D + DB - 1) / DB;
  if (nb <= 1) return 1;
  if (splits >= 1) return splits < nb ? splits : nb;
  // the library's choice: about eight workgroups per CU (two or more are resident; many short ones leave a small
  // tail), at most 64 ranges (the partials are ranges x k x V)
  const int64_t tblocks = (V + TB - 1) / TB;
  int64_t want = tblocks > 0 ? (8 * SP_CUS + tblocks - 1) / tblocks : 1;
  if (want > nb) want = nb;
  if (want > 64) want = 64;
  return want < 1 ? 1 : want;
}

struct Layout {
  size_t a_bytes, b_bytes, p_bytes;
  int64_t ranges;
  size_t total() const { return a_bytes + b_bytes + p_bytes; }
};

Layout lda_layout(size_t sz, int64_t V, int64_t D, int64_t k, int32_t splits) {
  Layout l;
  const int64_t kp = 16 * lda_kt(k);
  l.ranges = lda_ranges(V, D, k, splits);
  l.a_bytes = sp_align256((size_t)(V > 0 ? V : 1) * kp * sz);
  l.b_bytes = sp_align256((size_t)(D > 0 ? D : 1) * kp * sz);
  l.p_bytes = l.ranges > 1 ? sp_align256((size_t)l.ranges * k * V * sz) : 0;
  return l;
}

template <typename T, int KT>
int lda_launch(const T* X, int64_t ldx, int64_t V, int64_t D, const T* N, int64_t ldn, int64_t k, double alpha,
               double eta, int32_t iters, T* delta, int64_t ldd, T* doc_topics, int64_t ldt, T* A, T* Bst, T* P,
               int64_t ranges, hipStream_t st) {
  constexpr int KP = 16 * KT, TC = Cfg<T, KT>::TC, DC = Cfg<T, KT>::DC;
  const int64_t nb = (D + DB - 1) / DB, tblocks = (V + TB - 1) / TB;
  if (V > 0) {
    hipLaunchKernelGGL(lda_prep_kernel<T>, dim3(KP), dim3(256), 0, st, N, ldn, V, k, KP, (T)eta, A);
    SP_CHECK_LAUNCH();
  }
  if (D > 0) {
    const size_t smem = (size_t)(KP * PD + KP * (TC + 4) + TC * PD + DB) * sizeof(T) + DB * sizeof(int);
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lda_gamma_kernel<T, KT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL((lda_gamma_kernel<T, KT>), dim3((unsigned)nb), dim3(256), smem, st, X, ldx, V, D, A, k, (T)alpha,
                       (int)iters, delta ? Bst : (T*)nullptr, doc_topics, ldt);
    SP_CHECK_LAUNCH();
  }
  if (!delta || V == 0) return 0;
  if (D > 0) {
    const size_t smem = (size_t)(KP * PD + KP * (DC + 4) + TB * (DC + 4)) * sizeof(T);
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lda_delta_kernel<T, KT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    if (ranges > 1)
      hipLaunchKernelGGL((lda_delta_kernel<T, KT>), dim3((unsigned)(tblocks * ranges)), dim3(256), smem, st, X, ldx, V, D,
                         A, k, Bst, tblocks, ranges, P, V, k * V);
    else
      hipLaunchKernelGGL((lda_delta_kernel<T, KT>), dim3((unsigned)tblocks), dim3(256), smem, st, X, ldx, V, D, A, k, Bst,
                         tblocks, (int64_t)1, delta, ldd, (int64_t)0);
    SP_CHECK_LAUNCH();
  }
  // delta[t, j] <- P_0[t, j] + P_1[t, j] + ... in ascending order; 0 with no range at all (D = 0)
  if (D == 0 || ranges > 1)
    return sp_partial_sum<T>(P, D == 0 ? (int64_t)0 : ranges, k, V, delta, ldd, (const T*)nullptr, 0, (T*)nullptr, st);
  return 0;
}

template <typename T>
int lda_run(const T* X, int64_t ldx, int64_t V, int64_t D, const T* N, int64_t ldn, int64_t k, double alpha, double eta,
            int32_t iters, int32_t splits, T* delta, int64_t ldd, T* doc_topics, int64_t ldt, void* ws, size_t ws_bytes,
            hipStream_t st) {
  const Layout l = lda_layout(sizeof(T), V, D, k, splits);
  if (!ws || ws_bytes < l.total()) SP_FAIL("sp_lda_step: workspace of %zu bytes, %zu needed", ws_bytes, l.total());
  const int64_t nb = (D + DB - 1) / DB, tblocks = (V + TB - 1) / TB;
  if (nb > 0x7fffffffLL || (double)tblocks * (double)l.ranges > 2147483647.0)
    SP_FAIL("sp_lda_step: V=%lld D=%lld are too many workgroups for one launch", (long long)V, (long long)D);
  unsigned char* wsb = reinterpret_cast<unsigned char*>(ws);
  T* A = reinterpret_cast<T*>(wsb);
  T* Bst = reinterpret_cast<T*>(wsb + l.a_bytes);
  T* P = reinterpret_cast<T*>(wsb + l.a_bytes + l.b_bytes);
  switch (lda_kt(k)) {
    case 1:
      return lda_launch<T, 1>(X, ldx, V, D, N, ldn, k, alpha, eta, iters, delta, ldd, doc_topics, ldt, A, Bst, P, l.ranges, st);
    case 2:
      return lda_launch<T, 2>(X, ldx, V, D, N, ldn, k, alpha, eta, iters, delta, ldd, doc_topics, ldt, A, Bst, P, l.ranges, st);
    case 4:
      return lda_launch<T, 4>(X, ldx, V, D, N, ldn, k, alpha, eta, iters, delta, ldd, doc_topics, ldt, A, Bst, P, l.ranges, st);
    default:
      return lda_launch<T, 8>(X, ldx, V, D, N, ldn, k, alpha, eta, iters, delta, ldd, doc_topics, ldt, A, Bst, P, l.ranges, st);
  }
}

bool lda_shape_ok(int64_t V, int64_t D, int64_t k, int32_t iters, int32_t splits) {
  return V >= 0 && D >= 0 && k >= 1 && k <= SP_LDA_MAX_K && iters >= 1 && splits >= 0;
}

}  // namespace

extern "C" size_t sp_lda_step_workspace_bytes(int32_t dtype, int64_t V, int64_t D, int64_t k, int32_t iters,
                                              int32_t splits) {
  if ((dtype != SP_F32 && dtype != SP_F64) || !lda_shape_ok(V, D, k, iters, splits)) return 0;
  return lda_layout(sp_dtype_size(dtype), V, D, k, splits).total();
}

extern "C" int sp_lda_step(int32_t dtype, const void* d_X, int64_t ldx, int64_t V, int64_t D, const void* d_N,
                           int64_t ldn, int64_t k, double alpha, double eta, int32_t iters, int32_t splits,
                           void* d_delta, int64_t ldd, void* d_doc_topics, int64_t ldt, void* d_ws, size_t ws_bytes,
                           void* stream) {
  return sp_float_dispatch("sp_lda_step", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k < 1 || k > SP_LDA_MAX_K) SP_FAIL("sp_lda_step: k = %lld must be in 1 .. %d", (long long)k, SP_LDA_MAX_K);
    if (iters < 1) SP_FAIL("sp_lda_step: iters = %d must be at least 1", (int)iters);
    if (!(alpha > 0.0) || std::isinf(alpha)) SP_FAIL("sp_lda_step: alpha = %g must be finite and > 0", alpha);
    if (!(eta > 0.0) || std::isinf(eta)) SP_FAIL("sp_lda_step: eta = %g must be finite and > 0", eta);
    if (!lda_shape_ok(V, D, k, iters, splits) || ldx < D || ldn < V || (d_delta && ldd < V) || (d_doc_topics && ldt < k))
      SP_FAIL("sp_lda_step: bad shape V=%lld D=%lld k=%lld ldx=%lld ldn=%lld ldd=%lld ldt=%lld splits=%d", (long long)V,
              (long long)D, (long long)k, (long long)ldx, (long long)ldn, (long long)ldd, (long long)ldt, (int)splits);
    if (V > 0 && (!d_N || (D > 0 && !d_X))) SP_FAIL("sp_lda_step: X and N are required");
    return lda_run<T>((const T*)d_X, ldx, V, D, (const T*)d_N, ldn, k, alpha, eta, iters, splits, (T*)d_delta, ldd,
                      (T*)d_doc_topics, ldt, d_ws, ws_bytes, (hipStream_t)stream);
  });
}
