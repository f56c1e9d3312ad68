// The k most similar items of every item by cosine similarity, similarity and selection fused: the two shuffles of the
// reference's item-based recommender
//   spartan/examples/cf/item_recommender.py   _similarity_mapper (:70-75: S = L^T . R / (|L| |R|^T), nan_to_num, into
//                                             the N x N table) and _select_most_k_similar_mapper (:100: argpartsort)
// without the table.  The contract is in include/spartan_hip_cf.h.  Two kernels, shaped as knn.hip's:
//   cf_scan_kernel    a workgroup of 256 threads = 64 target items x one range of the source items.  Items are the
//                     COLUMNS of the row-major rating table, so a chunk of 16 users x 64 items is sixteen contiguous
//                     64-element runs for either operand: lane l of wave w loads item l of users w, w + 4, w + 8,
//                     w + 12 of the chunk and stores it user-major with a row pitch of 68 (reads are 16-byte, 16-byte
//                     aligned; the next chunk is in flight in registers while this one is used).  No transpose.  Thread
//                     (ty, tx) of the 16 x 16 grid holds the 4 x 4 inner products of targets 4 ty .. 4 ty + 3 and
//                     sources 4 tx .. 4 tx + 3; every one is ONE accumulator that takes t_u * s_u for u = 0, 1, ...
//                     in turn.  When the last user is in, the thread finishes its 16 similarities (one product of
//                     norms, one division, nan_to_num).  Wave w holds targets 16 w .. 16 w + 15 and nobody else
//                     does: their candidate lists (LDS, sorted by (similarity descending, index), k entries each) are
//                     private to the wave and selection needs no workgroup barrier.
//   cf_merge_kernel   one wave per row over unordered candidates, the same list and the same insertion.
// Selection is knn.hip's with the order turned round: a lane compares a finished similarity with the k-th best of its
// target -- the full key (similarity, index), so the result does not depend on the order in which sources arrive --
// and the wave then takes the survivors one at a time (ballot), checks each again against the list as it now stands
// and inserts it together.  The list code is a copy of knn.hip's with `better` in the place of `less` and -inf in the
// place of +inf: knn.hip's device code is pinned as it is (profiles/extras_shared_pieces_notes.md), so the two are
// not folded into one here.
#include <limits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_cf.h"

namespace {

constexpr int TB = 64;        // targets per workgroup
constexpr int SB = 64;        // sources per pass
constexpr int UC = 16;        // users per chunk
constexpr int PITCH = 68;     // elements between the user rows of a staged chunk (64 + 4: 16-byte aligned rows)

// the total order on (similarity descending, index ascending); false whenever a is NaN
template <typename T, typename I>
__device__ __forceinline__ bool key_better(T a, I ia, T b, I ib) {
  return a > b || (a == b && ia < ib);
}

template <typename T, typename I>
__device__ __forceinline__ void list_clear(T* ls, I* li, int n, int lane) {
  for (int e = lane; e < n; e += 64) {
    ls[e] = -std::numeric_limits<T>::infinity();     // (no finished similarity is -inf: nan_to_num has seen it)
    li[e] = std::numeric_limits<I>::max();           // (no item has this index: after every real key's tie-break)
  }
}

// The whole wave inserts (sv, iv) -- wave-uniform, better than the list's last key -- into the sorted list of k <= 128.
template <typename T, typename I>
__device__ __forceinline__ void list_insert(T* ls, I* li, int k, int lane, T sv, I iv) {
  const bool h0 = lane < k, h1 = lane + 64 < k;
  T s0 = 0, s1 = 0;
  I i0 = 0, i1 = 0;
  if (h0) { s0 = ls[lane]; i0 = li[lane]; }
  if (h1) { s1 = ls[lane + 64]; i1 = li[lane + 64]; }
  const bool bt0 = h0 && key_better(s0, i0, sv, iv), bt1 = h1 && key_better(s1, i1, sv, iv);
  const int p = __popcll(__ballot(bt0)) + __popcll(__ballot(bt1));     // entries before the new key: its position
  sp_wave_sync();                                                      // (every read above before any write below)
  if (h0 && !bt0 && lane + 1 < k) { ls[lane + 1] = s0; li[lane + 1] = i0; }
  if (h1 && !bt1 && lane + 65 < k) { ls[lane + 65] = s1; li[lane + 65] = i1; }
  if (lane == 0 && p < k) { ls[p] = sv; li[p] = iv; }
  sp_wave_sync();
}

// np.nan_to_num: NaN -> +0, +inf -> the largest finite, -inf -> the most negative finite
template <typename T>
__device__ __forceinline__ T nan_to_num(T v) {
  if (v != v) return (T)0;
  if (v == std::numeric_limits<T>::infinity()) return std::numeric_limits<T>::max();
  if (v == -std::numeric_limits<T>::infinity()) return std::numeric_limits<T>::lowest();
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void cf_scan_kernel(const T* __restrict__ Tg, int64_t ldt, const T* __restrict__ tnorm,
                                                      int64_t m, const T* __restrict__ Sg, int64_t lds,
                                                      const T* __restrict__ snorm, int64_t ns, int64_t users, int k,
                                                      int64_t index_offset, int splits, T* __restrict__ out_s,
                                                      int64_t* __restrict__ out_i, int64_t ldo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cf_smem[];
  T* ts = reinterpret_cast<T*>(cf_smem);                   // [UC][PITCH]
  T* ss = ts + UC * PITCH;                                 // [UC][PITCH]
  T* cs = ss + UC * PITCH;                                 // [TB][k]
  int32_t* ci = reinterpret_cast<int32_t*>(cs + (size_t)TB * k);      // [TB][k]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = tid >> 4, tx = tid & 15;
  const int64_t tblock = (int64_t)blockIdx.x / splits;
  const int split = (int)((int64_t)blockIdx.x % splits);
  const int64_t t0 = tblock * TB;
  const int64_t pb = (int64_t)split * ns / splits, pe = (int64_t)(split + 1) * ns / splits;

  list_clear(cs + (size_t)wave * 16 * k, ci + (size_t)wave * 16 * k, 16 * k, lane);
  sp_wave_sync();

  T tn[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) tn[a] = (t0 + ty * 4 + a < m) ? tnorm[t0 + ty * 4 + a] : (T)0;

  // staging: thread (user wave + 4 i, item lane), i = 0 .. 3, of the [16 users][64 items] chunk
  const int64_t nchunks = (users + UC - 1) / UC;
  const bool t_in = t0 + lane < m;
  T tv_next[4], sv_next[4];

  for (int64_t p0 = pb; p0 < pe; p0 += SB) {
    T acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = (T)0;

    const bool s_in = p0 + lane < pe;
    auto fetch = [&](int64_t c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t u = c * UC + wave + 4 * i;
        tv_next[i] = (u < users && t_in) ? Tg[u * ldt + t0 + lane] : (T)0;
        sv_next[i] = (u < users && s_in) ? Sg[u * lds + p0 + lane] : (T)0;
      }
    };
    if (nchunks > 0) fetch(0);
    for (int64_t c = 0; c < nchunks; ++c) {
      __syncthreads();                    // the previous chunk has been read by everyone
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ts[(wave + 4 * i) * PITCH + lane] = tv_next[i];
        ss[(wave + 4 * i) * PITCH + lane] = sv_next[i];
      }
      __syncthreads();
      if (c + 1 < nchunks) fetch(c + 1);
      const int un = (int)((users - c * UC) < UC ? (users - c * UC) : UC);
      if (un == UC) {
#pragma unroll 4
        for (int u = 0; u < UC; ++u) {
          const Vec4<T> tv = *reinterpret_cast<const Vec4<T>*>(ts + u * PITCH + ty * 4);
          const Vec4<T> sv = *reinterpret_cast<const Vec4<T>*>(ss + u * PITCH + tx * 4);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + tv.v[a] * sv.v[b];
        }
      } else {
        for (int u = 0; u < un; ++u) {
          const Vec4<T> tv = *reinterpret_cast<const Vec4<T>*>(ts + u * PITCH + ty * 4);
          const Vec4<T> sv = *reinterpret_cast<const Vec4<T>*>(ss + u * PITCH + tx * 4);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + tv.v[a] * sv.v[b];
        }
      }
    }

    // the similarities: one product of norms, one division, nan_to_num
    T sn[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) sn[b] = (p0 + tx * 4 + b < pe) ? snorm[p0 + tx * 4 + b] : (T)0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = nan_to_num(acc[a][b] / (tn[a] * sn[b]));

    // selection: the lists of targets 16 wave .. 16 wave + 15 belong to this wave alone
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = ty * 4 + a;
      const T ths = cs[(size_t)row * k + k - 1];
      const int32_t thi = ci[(size_t)row * k + k - 1];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t p = p0 + tx * 4 + b;
        const bool mine = (t0 + row < m) && (p < pe) && key_better(acc[a][b], (int32_t)p, ths, thi);
        unsigned long long todo = __ballot(mine);
        while (todo) {
          const int src = __ffsll(todo) - 1;
          todo &= todo - 1;
          const T sv = __shfl(acc[a][b], src);
          const int srow = (wave * 4 + (src >> 4)) * 4 + a;
          const int32_t iv = (int32_t)(p0 + (src & 15) * 4 + b);
          T* ls = cs + (size_t)srow * k;
          int32_t* li = ci + (size_t)srow * k;
          if (key_better(sv, iv, ls[k - 1], li[k - 1])) list_insert(ls, li, k, lane, sv, iv);
        }
      }
    }
  }

  sp_wave_sync();
  for (int r = 0; r < 16; ++r) {
    const int row = wave * 16 + r;
    if (t0 + row >= m) break;
    T* os = out_s + (t0 + row) * ldo + (int64_t)split * k;
    int64_t* oi = out_i + (t0 + row) * ldo + (int64_t)split * k;
    for (int e = lane; e < k; e += 64) {
      const int32_t i = ci[(size_t)row * k + e];
      os[e] = cs[(size_t)row * k + e];
      oi[e] = i == std::numeric_limits<int32_t>::max() ? (int64_t)-1 : index_offset + i;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cf_merge_kernel(const T* __restrict__ cand_s, const int64_t* __restrict__ cand_i,
                                                       int64_t ldc, int64_t m, int64_t cands, int k,
                                                       T* __restrict__ out_s, int64_t* __restrict__ out_i) {
  __shared__ T ls_all[4][SP_CF_MAX_K];
  __shared__ int64_t li_all[4][SP_CF_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= m) return;                          // (a whole wave; nothing below synchronises the workgroup)
  T* ls = ls_all[wave];
  int64_t* li = li_all[wave];
  list_clear(ls, li, k, lane);
  sp_wave_sync();
  const T* rs = cand_s + row * ldc;
  const int64_t* ri = cand_i + row * ldc;
  for (int64_t base = 0; base < cands; base += 64) {
    const int64_t c = base + lane;
    T sv0 = 0;
    int64_t iv0 = -1;
    if (c < cands) { sv0 = rs[c]; iv0 = ri[c]; }
    const bool mine = iv0 >= 0 && key_better(sv0, iv0, ls[k - 1], li[k - 1]);
    unsigned long long todo = __ballot(mine);
    while (todo) {
      const int src = __ffsll(todo) - 1;
      todo &= todo - 1;
      const T sv = __shfl(sv0, src);
      const int64_t iv = __shfl(iv0, src);
      if (key_better(sv, iv, ls[k - 1], li[k - 1])) list_insert(ls, li, k, lane, sv, iv);
    }
  }
  sp_wave_sync();
  for (int e = lane; e < k; e += 64) {
    const int64_t i = li[e];
    out_s[row * k + e] = ls[e];
    out_i[row * k + e] = i == std::numeric_limits<int64_t>::max() ? (int64_t)-1 : i;
  }
}

// the number of ranges the sources are cut into
int64_t cf_ranges(int64_t m, int64_t ns, int32_t k, int32_t splits) {
  if (ns <= 0) return 1;
  if (splits >= 1) return splits < ns ? splits : ns;
  // the library's choice, from (m, ns, k) alone: about two workgroups per CU, every range at least one source block
  // and 4 k sources long, so that the merge (ranges x k candidates per target) stays small beside the scan, whose cost
  // per source grows with the number of users; then the fewest ranges that need the same number of passes of 64
  // sources, so that no range ends in a nearly empty pass (800 sources: 13 ranges of 61 or 62, one pass each)
  const int64_t tblocks = (m + TB - 1) / TB;
  int64_t want = tblocks > 0 ? (2 * SP_CUS + tblocks - 1) / tblocks : 1;
  const int64_t floor_len = 4 * (int64_t)k > SB ? 4 * (int64_t)k : SB;
  const int64_t most = (ns + floor_len - 1) / floor_len;
  if (want > most) want = most;
  if (want > 64) want = 64;
  if (want <= 1) return 1;
  const int64_t longest = (ns + want - 1) / want, passes = (longest + SB - 1) / SB;
  return (ns + SB * passes - 1) / (SB * passes);
}

// the workspace: with more than one range, every range's k candidates per target -- similarities, then indices
struct Layout {
  int64_t ranges;
  size_t s_bytes, i_bytes;
  size_t total() const { return s_bytes + i_bytes; }
};

Layout cf_layout(size_t sz, int64_t m, int64_t ns, int32_t k, int32_t splits) {
  Layout l;
  l.ranges = cf_ranges(m, ns, k, splits);
  l.s_bytes = l.ranges > 1 ? sp_align256((size_t)m * l.ranges * k * sz) : 0;
  l.i_bytes = l.ranges > 1 ? (size_t)m * l.ranges * k * sizeof(int64_t) : 0;
  return l;
}

template <typename T>
int cf_merge_launch(const T* cs, const int64_t* ci, int64_t ldc, int64_t m, int64_t cands, int32_t k, T* os, int64_t* oi,
                    hipStream_t st) {
  const int64_t blocks = (m + 3) / 4;
  if (blocks > 0x7fffffffLL) SP_FAIL("sp_item_topk_merge: %lld rows are too many for one launch", (long long)m);
  hipLaunchKernelGGL(cf_merge_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, cs, ci, ldc, m, cands, (int)k, os, oi);
  SP_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int cf_run(const T* Tg, int64_t ldt, const T* tnorm, int64_t m, const T* Sg, int64_t lds, const T* snorm, int64_t ns,
           int64_t users, int32_t k, int64_t index_offset, int32_t splits, T* os, int64_t* oi, void* ws, size_t ws_bytes,
           hipStream_t st) {
  const Layout l = cf_layout(sizeof(T), m, ns, k, splits);
  const int64_t ranges = l.ranges, tblocks = (m + TB - 1) / TB;
  if (tblocks * ranges > 0x7fffffffLL) SP_FAIL("sp_item_topk: %lld targets x %lld ranges are too many for one launch",
                                               (long long)m, (long long)ranges);
  T* ss = os;
  int64_t* si = oi;
  int64_t ldo = k;
  if (ranges > 1) {
    if (!ws || ws_bytes < l.total()) SP_FAIL("sp_item_topk: workspace of %zu bytes, %zu needed", ws_bytes, l.total());
    ss = reinterpret_cast<T*>(ws);
    si = reinterpret_cast<int64_t*>(reinterpret_cast<unsigned char*>(ws) + l.s_bytes);
    ldo = ranges * k;
  }
  const size_t smem = 2 * UC * PITCH * sizeof(T) + (size_t)TB * k * (sizeof(T) + sizeof(int32_t));
  SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cf_scan_kernel<T>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(cf_scan_kernel<T>, dim3((unsigned)(tblocks * ranges)), dim3(256), smem, st, Tg, ldt, tnorm, m, Sg, lds,
                     snorm, ns, users, (int)k, index_offset, (int)ranges, ss, si, ldo);
  SP_CHECK_LAUNCH();
  if (ranges > 1) return cf_merge_launch<T>(ss, si, ldo, m, ldo, k, os, oi, st);
  return 0;
}

}  // namespace

extern "C" size_t sp_item_topk_workspace_bytes(int32_t dtype, int64_t users, int64_t m, int64_t ns, int32_t k,
                                               int32_t splits) {
  (void)users;
  if ((dtype != SP_F32 && dtype != SP_F64) || m <= 0 || k < 1 || k > SP_CF_MAX_K || splits < 0) return 0;
  return cf_layout(sp_dtype_size(dtype), m, ns, k, splits).total();
}

extern "C" int sp_item_topk(int32_t dtype, const void* d_T, int64_t ldt, const void* d_tnorm, int64_t m, const void* d_S,
                            int64_t lds, const void* d_snorm, int64_t ns, int64_t users, int32_t k, int64_t index_offset,
                            int32_t splits, void* d_sim, int64_t* d_idx, void* d_ws, size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_item_topk", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k < 1 || k > SP_CF_MAX_K) SP_FAIL("sp_item_topk: k = %d is outside 1 .. %d", (int)k, SP_CF_MAX_K);
    if (m < 0 || ns < 0 || users < 0 || ldt < m || lds < ns || splits < 0)
      SP_FAIL("sp_item_topk: bad shape users=%lld m=%lld ns=%lld ldt=%lld lds=%lld splits=%d", (long long)users,
              (long long)m, (long long)ns, (long long)ldt, (long long)lds, (int)splits);
    if (ns > 0x7ffffffeLL) SP_FAIL("sp_item_topk: %lld sources in one call (at most 2^31 - 2; search column ranges with "
                                   "index_offset and merge)", (long long)ns);
    if (m == 0) return 0;
    if (!d_sim || !d_idx || !d_tnorm || (ns > 0 && !d_snorm) || (users > 0 && (!d_T || (ns > 0 && !d_S))))
      SP_FAIL("sp_item_topk: operands and results are required (users=%lld m=%lld ns=%lld)", (long long)users,
              (long long)m, (long long)ns);
    return cf_run<T>((const T*)d_T, ldt, (const T*)d_tnorm, m, (const T*)d_S, lds, (const T*)d_snorm, ns, users, k,
                     index_offset, splits, (T*)d_sim, d_idx, d_ws, ws_bytes, (hipStream_t)stream);
  });
}

extern "C" int sp_item_topk_merge(int32_t dtype, const void* d_cand_sim, const int64_t* d_cand_idx, int64_t ldc, int64_t m,
                                  int64_t cands, int32_t k, void* d_sim, int64_t* d_idx, void* stream) {
  return sp_float_dispatch("sp_item_topk_merge", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (k < 1 || k > SP_CF_MAX_K) SP_FAIL("sp_item_topk_merge: k = %d is outside 1 .. %d", (int)k, SP_CF_MAX_K);
    if (m < 0 || cands < 0 || ldc < cands)
      SP_FAIL("sp_item_topk_merge: bad shape m=%lld cands=%lld ldc=%lld", (long long)m, (long long)cands, (long long)ldc);
    if (m == 0) return 0;
    return cf_merge_launch<T>((const T*)d_cand_sim, d_cand_idx, ldc, m, cands, k, (T*)d_sim, d_idx, (hipStream_t)stream);
  });
}
