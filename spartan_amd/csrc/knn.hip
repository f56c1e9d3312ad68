// k nearest neighbours by squared Euclidean distance, distance and selection fused: the per-tile search of the
// reference's NearestNeighbors
//   spartan/examples/sklearn/neighbors/unsupervised.py   _knn_mapper (:43-48: scikit-learn's trees on one tile of X)
//                                                        kneighbors (:140-142: argsort of the tiles' candidates)
// The contract is in include/spartan_hip_knn.h.  Two kernels:
//   knn_scan_kernel   a workgroup of 256 threads = 64 queries x one range of the points.  Points pass through LDS 64 at
//                     a time, both operands in chunks of 16 features stored feature-major with a row pitch of 68 (reads
//                     are 16-byte, 16-byte aligned; the next chunk is in flight in registers while this one is
//                     used): sp_d2_tile of sp_extras_common.hpp, written out in this kernel (the comment there says
//                     why).  Thread (ty, tx) of the 16 x 16 grid holds the 4 x 4 distances of queries 4 ty .. 4 ty + 3
//                     and points 4 tx .. 4 tx + 3; every one is ONE accumulator that takes (q_j - x_j)^2 for j = 0, 1, ...
//                     in turn.  Wave w therefore holds queries 16 w .. 16 w + 15 and nobody else does: their candidate
//                     lists (LDS, sorted by (d2, index), k entries each) are private to the wave and selection needs
//                     no workgroup barrier.
//   knn_merge_kernel  one wave per row over m unordered candidates, the same list and the same insertion.
// Selection: a lane compares a finished distance with the k-th best of its query -- the full key (d2, index), so the
// result does not depend on the order in which points arrive -- and the wave then takes the survivors one at a time
// (ballot), checks each again against the list as it now stands and inserts it together: every lane reads its one or
// two list entries, a ballot counts those below the new key, the others move up by one.  Survivors are rare once a
// list is full (about k ln(n / k) per query over n points).
#include <limits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_knn.h"

namespace {

constexpr int QB = 64;        // queries per workgroup
constexpr int PB = 64;        // points per pass
constexpr int DC = SP_D2_DC;        // features per chunk of the distance tile
constexpr int PITCH = SP_D2_PITCH;  // elements between the feature rows of a staged chunk

// the total order on (d2, index); false whenever a is NaN
template <typename T, typename I>
__device__ __forceinline__ bool key_less(T a, I ia, T b, I ib) {
  return a < b || (a == b && ia < ib);
}

template <typename T, typename I>
__device__ __forceinline__ void list_clear(T* ld, I* li, int n, int lane) {
  for (int e = lane; e < n; e += 64) {
    ld[e] = std::numeric_limits<T>::infinity();
    li[e] = std::numeric_limits<I>::max();          // (no point has this index: below every real key's tie-break)
  }
}

// The whole wave inserts (dv, iv) -- wave-uniform, below the list's last key -- into the sorted list of k <= 128 entries.
template <typename T, typename I>
__device__ __forceinline__ void list_insert(T* ld, I* li, int k, int lane, T dv, I iv) {
  const bool h0 = lane < k, h1 = lane + 64 < k;
  T d0 = 0, d1 = 0;
  I i0 = 0, i1 = 0;
  if (h0) { d0 = ld[lane]; i0 = li[lane]; }
  if (h1) { d1 = ld[lane + 64]; i1 = li[lane + 64]; }
  const bool lt0 = h0 && key_less(d0, i0, dv, iv), lt1 = h1 && key_less(d1, i1, dv, iv);
  const int p = __popcll(__ballot(lt0)) + __popcll(__ballot(lt1));     // entries below the new key: its position
  sp_wave_sync();                                                      // (every read above before any write below)
  if (h0 && !lt0 && lane + 1 < k) { ld[lane + 1] = d0; li[lane + 1] = i0; }
  if (h1 && !lt1 && lane + 65 < k) { ld[lane + 65] = d1; li[lane + 65] = i1; }
  if (lane == 0 && p < k) { ld[p] = dv; li[p] = iv; }
  sp_wave_sync();
}

template <typename T>
__global__ __launch_bounds__(256) void knn_scan_kernel(const T* __restrict__ Q, int64_t ldq, int64_t nq,
                                                       const T* __restrict__ X, int64_t ldx, int64_t np, int64_t d,
                                                       int k, int64_t index_offset, int splits, T* __restrict__ out_d,
                                                       int64_t* __restrict__ out_i, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  T* qs = reinterpret_cast<T*>(knn_smem);                  // [DC][PITCH]
  T* xs = qs + DC * PITCH;                                 // [DC][PITCH]
  T* cd = xs + DC * PITCH;                                 // [QB][k]
  int32_t* ci = reinterpret_cast<int32_t*>(cd + (size_t)QB * k);      // [QB][k]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = tid >> 4, tx = tid & 15;
  const int64_t qblock = (int64_t)blockIdx.x / splits;
  const int split = (int)((int64_t)blockIdx.x % splits);
  const int64_t q0 = qblock * QB;
  const int64_t pb = (int64_t)split * np / splits, pe = (int64_t)(split + 1) * np / splits;

  list_clear(cd + (size_t)wave * 16 * k, ci + (size_t)wave * 16 * k, 16 * k, lane);
  sp_wave_sync();

  // The distance tile below is sp_d2_tile (sp_extras_common.hpp) written out: the same staging, the same order of
  // accumulation, with `pe`, the range's end, in the place of its k.  A deliberate copy: called as a function the tile
  // costs this kernel 12 VGPRs in fp64 and 1 - 4 % of its time (fp64; up to 2 % in fp32 at d = 16), measured in
  // profiles/extras_shared_pieces_notes.md.  A change to either copy belongs in both.
  // staging: thread (lr0 + 16 i, lj), i = 0 .. 3, of the [64 rows][16 features] chunk: a row's 16 features are one
  // 64- or 128-byte run for 16 consecutive lanes
  const int lj = tid & 15, lr0 = tid >> 4;
  const int nchunks = (int)((d + DC - 1) / DC);
  T qn[4], xn[4];

  for (int64_t p0 = pb; p0 < pe; p0 += PB) {
    T acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = (T)0;

    auto fetch = [&](int c) {
      const int64_t col = (int64_t)c * DC + lj;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t qr = q0 + lr0 + 16 * i, pr = p0 + lr0 + 16 * i;
        qn[i] = (col < d && qr < nq) ? Q[qr * ldq + col] : (T)0;
        xn[i] = (col < d && pr < pe) ? X[pr * ldx + col] : (T)0;
      }
    };
    if (nchunks > 0) fetch(0);
    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();                    // the previous chunk has been read by everyone
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qs[lj * PITCH + lr0 + 16 * i] = qn[i];
        xs[lj * PITCH + lr0 + 16 * i] = xn[i];
      }
      __syncthreads();
      if (c + 1 < nchunks) fetch(c + 1);
      const int jn = (int)((d - (int64_t)c * DC) < DC ? (d - (int64_t)c * DC) : DC);
      if (jn == DC) {
#pragma unroll 4
        for (int j = 0; j < DC; ++j) {
          const Vec4<T> qv = *reinterpret_cast<const Vec4<T>*>(qs + j * PITCH + ty * 4);
          const Vec4<T> xv = *reinterpret_cast<const Vec4<T>*>(xs + j * PITCH + tx * 4);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const T t = qv.v[a] - xv.v[b];
              acc[a][b] = acc[a][b] + t * t;
            }
        }
      } else {
        for (int j = 0; j < jn; ++j) {
          const Vec4<T> qv = *reinterpret_cast<const Vec4<T>*>(qs + j * PITCH + ty * 4);
          const Vec4<T> xv = *reinterpret_cast<const Vec4<T>*>(xs + j * PITCH + tx * 4);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const T t = qv.v[a] - xv.v[b];
              acc[a][b] = acc[a][b] + t * t;
            }
        }
      }
    }

    // selection: the lists of rows 16 wave .. 16 wave + 15 belong to this wave alone
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = ty * 4 + a;
      const T thd = cd[(size_t)row * k + k - 1];
      const int32_t thi = ci[(size_t)row * k + k - 1];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t p = p0 + tx * 4 + b;
        const bool mine = (q0 + row < nq) && (p < pe) && key_less(acc[a][b], (int32_t)p, thd, thi);
        unsigned long long todo = __ballot(mine);
        while (todo) {
          const int src = __ffsll(todo) - 1;
          todo &= todo - 1;
          const T dv = __shfl(acc[a][b], src);
          const int srow = (wave * 4 + (src >> 4)) * 4 + a;
          const int32_t iv = (int32_t)(p0 + (src & 15) * 4 + b);
          T* ld = cd + (size_t)srow * k;
          int32_t* li = ci + (size_t)srow * k;
          if (key_less(dv, iv, ld[k - 1], li[k - 1])) list_insert(ld, li, k, lane, dv, iv);
        }
      }
    }
  }

  sp_wave_sync();
  for (int r = 0; r < 16; ++r) {
    const int row = wave * 16 + r;
    if (q0 + row >= nq) break;
    T* od = out_d + (q0 + row) * ldo + (int64_t)split * k;
    int64_t* oi = out_i + (q0 + row) * ldo + (int64_t)split * k;
    for (int e = lane; e < k; e += 64) {
      const int32_t i = ci[(size_t)row * k + e];
      od[e] = cd[(size_t)row * k + e];
      oi[e] = i == std::numeric_limits<int32_t>::max() ? (int64_t)-1 : index_offset + i;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void knn_merge_kernel(const T* __restrict__ cand_d, const int64_t* __restrict__ cand_i,
                                                        int64_t ldc, int64_t nq, int64_t m, int k,
                                                        T* __restrict__ out_d, int64_t* __restrict__ out_i) {
  __shared__ T ld_all[4][SP_KNN_MAX_K];
  __shared__ int64_t li_all[4][SP_KNN_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= nq) return;                         // (a whole wave; nothing below synchronises the workgroup)
  T* ld = ld_all[wave];
  int64_t* li = li_all[wave];
  list_clear(ld, li, k, lane);
  sp_wave_sync();
  const T* rd = cand_d + row * ldc;
  const int64_t* ri = cand_i + row * ldc;
  for (int64_t base = 0; base < m; base += 64) {
    const int64_t c = base + lane;
    T dv0 = 0;
    int64_t iv0 = -1;
    if (c < m) { dv0 = rd[c]; iv0 = ri[c]; }
    const bool mine = iv0 >= 0 && key_less(dv0, iv0, ld[k - 1], li[k - 1]);
    unsigned long long todo = __ballot(mine);
    while (todo) {
      const int src = __ffsll(todo) - 1;
      todo &= todo - 1;
      const T dv = __shfl(dv0, src);
      const int64_t iv = __shfl(iv0, src);
      if (key_less(dv, iv, ld[k - 1], li[k - 1])) list_insert(ld, li, k, lane, dv, iv);
    }
  }
  sp_wave_sync();
  for (int e = lane; e < k; e += 64) {
    const int64_t i = li[e];
    out_d[row * k + e] = ld[e];
    out_i[row * k + e] = i == std::numeric_limits<int64_t>::max() ? (int64_t)-1 : i;
  }
}

// the number of ranges the points are cut into
int64_t knn_ranges(int64_t nq, int64_t np, int32_t k, int32_t splits) {
  if (np <= 0) return 1;
  if (splits >= 1) return splits < np ? splits : np;
  // the library's choice: about two workgroups per CU, every range long enough that its list fills early and the
  // merge (ranges x k candidates per query) stays small beside the scan
  const int64_t qblocks = (nq + QB - 1) / QB;
  int64_t want = qblocks > 0 ? (2 * SP_CUS + qblocks - 1) / qblocks : 1;
  const int64_t floor_len = 32 * (int64_t)k > 4096 ? 32 * (int64_t)k : 4096;
  const int64_t most = np / floor_len;
  if (want > most) want = most;
  if (want > 64) want = 64;
  return want < 1 ? 1 : want;
}

// the workspace: with more than one range, every range's k candidates per query -- distances, then indices
struct Layout {
  int64_t ranges;
  size_t d_bytes, i_bytes;
  size_t total() const { return d_bytes + i_bytes; }
};

Layout knn_layout(size_t sz, int64_t nq, int64_t np, int32_t k, int32_t splits) {
  Layout l;
  l.ranges = knn_ranges(nq, np, k, splits);
  l.d_bytes = l.ranges > 1 ? sp_align256((size_t)nq * l.ranges * k * sz) : 0;
  l.i_bytes = l.ranges > 1 ? (size_t)nq * l.ranges * k * sizeof(int64_t) : 0;
  return l;
}

template <typename T>
int knn_merge_launch(const T* cd, const int64_t* ci, int64_t ldc, int64_t nq, int64_t m, int32_t k, T* od, int64_t* oi,
                     hipStream_t st) {
  const int64_t blocks = (nq + 3) / 4;
  if (blocks > 0x7fffffffLL) SP_FAIL("sp_knn_merge: %lld rows are too many for one launch", (long long)nq);
  hipLaunchKernelGGL(knn_merge_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, cd, ci, ldc, nq, m, (int)k, od, oi);
  SP_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int knn_run(const T* Q, int64_t ldq, int64_t nq, const T* X, int64_t ldx, int64_t np, int64_t d, int32_t k,
            int64_t index_offset, int32_t splits, T* od, int64_t* oi, void* ws, size_t ws_bytes, hipStream_t st) {
  const Layout l = knn_layout(sizeof(T), nq, np, k, splits);
  const int64_t ranges = l.ranges, qblocks = (nq + QB - 1) / QB;
  if (qblocks * ranges > 0x7fffffffLL) SP_FAIL("sp_knn: %lld queries x %lld ranges are too many for one launch",
                                               (long long)nq, (long long)ranges);
  T* sd = od;
  int64_t* si = oi;
  int64_t ldo = k;
  if (ranges > 1) {
    if (!ws || ws_bytes < l.total()) SP_FAIL("sp_knn: workspace of %zu bytes, %zu needed", ws_bytes, l.total());
    sd = reinterpret_cast<T*>(ws);
    si = reinterpret_cast<int64_t*>(reinterpret_cast<unsigned char*>(ws) + l.d_bytes);
    ldo = ranges * k;
  }
  const size_t lds = 2 * DC * PITCH * sizeof(T) + (size_t)QB * k * (sizeof(T) + sizeof(int32_t));
  SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_scan_kernel<T>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(knn_scan_kernel<T>, dim3((unsigned)(qblocks * ranges)), dim3(256), lds, st, Q, ldq, nq, X, ldx, np, d,
                     (int)k, index_offset, (int)ranges, sd, si, ldo);
  SP_CHECK_LAUNCH();
  if (ranges > 1) return knn_merge_launch<T>(sd, si, ldo, nq, ldo, k, od, oi, st);
  return 0;
}

}  // namespace

extern "C" size_t sp_knn_workspace_bytes(int32_t dtype, int64_t nq, int64_t np, int64_t d, int32_t k, int32_t splits) {
  (void)d;
  if ((dtype != SP_F32 && dtype != SP_F64) || nq <= 0 || k < 1 || k > SP_KNN_MAX_K || splits < 0) return 0;
  return knn_layout(sp_dtype_size(dtype), nq, np, k, splits).total();
}

extern "C" int sp_knn(int32_t dtype, const void* d_Q, int64_t ldq, int64_t nq, const void* d_X, int64_t ldx, int64_t np,
                      int64_t d, int32_t k, int64_t index_offset, int32_t splits, void* d_dist2, int64_t* d_idx,
                      void* d_ws, size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_knn", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k < 1 || k > SP_KNN_MAX_K) SP_FAIL("sp_knn: k = %d is outside 1 .. %d", (int)k, SP_KNN_MAX_K);
    if (nq < 0 || np < 0 || d < 0 || ldq < d || ldx < d || splits < 0)
      SP_FAIL("sp_knn: bad shape nq=%lld np=%lld d=%lld ldq=%lld ldx=%lld splits=%d", (long long)nq, (long long)np,
              (long long)d, (long long)ldq, (long long)ldx, (int)splits);
    if (np > 0x7ffffffeLL) SP_FAIL("sp_knn: %lld points in one call (at most 2^31 - 2; search tiles with index_offset "
                                   "and merge)", (long long)np);
    if (nq == 0) return 0;
    return knn_run<T>((const T*)d_Q, ldq, nq, (const T*)d_X, ldx, np, d, k, index_offset, splits, (T*)d_dist2, d_idx, d_ws,
                      ws_bytes, (hipStream_t)stream);
  });
}

extern "C" int sp_knn_merge(int32_t dtype, const void* d_cand_dist2, const int64_t* d_cand_idx, int64_t ldc, int64_t nq,
                            int64_t m, int32_t k, void* d_dist2, int64_t* d_idx, void* stream) {
  return sp_float_dispatch("sp_knn_merge", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k < 1 || k > SP_KNN_MAX_K) SP_FAIL("sp_knn_merge: k = %d is outside 1 .. %d", (int)k, SP_KNN_MAX_K);
    if (nq < 0 || m < 0 || ldc < m) SP_FAIL("sp_knn_merge: bad shape nq=%lld m=%lld ldc=%lld", (long long)nq, (long long)m,
                                            (long long)ldc);
    if (nq == 0) return 0;
    return knn_merge_launch<T>((const T*)d_cand_dist2, d_cand_idx, ldc, nq, m, k, (T*)d_dist2, d_idx, (hipStream_t)stream);
  });
}
