// The tile body of the reference's Netflix SGD matrix factorisation, level-scheduled:
//   spartan/examples/netflix_core.pyx   _sgd_inner (a strictly sequential loop over a tile's ratings; every step reads
//                                       and rewrites one row of U and one row of M)
// The contract -- the sequence, the order of its dot, the plan's layout -- is in include/spartan_hip_mf.h.  Two ratings
// that share neither row nor column touch disjoint memory, so the entries of one level of the schedule run at once
// and give the sequential loop's bits.  Host code: sp_sgd_mf_plan (levels, counting sort, segments) and
// sp_sgd_mf_host (the plain loop).  Kernels:
//   mf_wide_kernel    one level of at least SP_MF_WIDE ratings, a launch of its own, no barrier
//   mf_narrow_kernel  a run of narrower levels in ONE workgroup, __syncthreads() between levels
// No atomics, no flags, no workgroup waits for another.  Contraction is off for the whole library (Makefile:
// -ffp-contract=off, host and device alike), which is what keeps (u * d) * lr and the adds apart.
#include <cmath>
#include <type_traits>
#include <vector>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_mf.h"

namespace {

constexpr int MF_BLOCK = 256;

// the views of a plan's bytes (host or device alike)
struct MfPlan {
  const int32_t *entry, *row, *col, *level_off, *segment;
};

inline int mf_lanes(int64_t f) { return f <= 16 ? 8 : (f <= 64 ? 16 : 64); }

// ---- the kernels ---------------------------------------------------------------------------------------------------
// one rating by the L lanes l = 0 .. L - 1 of a wave that all hold the same `pos`; K = the most elements per lane
template <typename T, int L, int K>
__device__ __forceinline__ void mf_rating(int64_t pos, int l, MfPlan p, const T* __restrict__ vals, T* U, int64_t ldu, T* M,
                                          int64_t ldm, int64_t m, int64_t n, int64_t nnz, int f, T lr, T* abs_err) {
  const int64_t e = p.entry[pos], i = p.row[pos], j = p.col[pos];
  // (a plan is built from a checked tile; a foreign block of bytes must not send a store out of bounds)
  if (e < 0 || e >= nnz || i < 0 || i >= m || j < 0 || j >= n) return;
  const T r = vals[e];
  T* up = U + i * ldu;
  T* mp = M + j * ldm;
  T u[K], v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = k * L + l;
    u[k] = (T)0;
    v[k] = (T)0;
    if (c < f) {
      u[k] = up[c];
      v[k] = mp[c];
    }
  }
  T s = (T)0;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k * L + l < f) s = s + u[k] * v[k];
  // the L lane sums as a balanced tree, partners at distance L / 2 first (addition commutes: every lane of the rating
  // ends with the same bits)
#pragma unroll
  for (int w = L / 2; w >= 1; w >>= 1) s = s + __shfl_xor(s, w);
  const T d = r - s;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = k * L + l;
    if (c < f) {
      up[c] = u[k] + (u[k] * d) * lr;
      mp[c] = v[k] + (v[k] * d) * lr;
    }
  }
  if (abs_err && l == 0) abs_err[e] = abs_t(d);
}

// the positions begin .. end - 1 of ONE level
template <typename T, int L, int K>
__global__ __launch_bounds__(MF_BLOCK) void mf_wide_kernel(int64_t begin, int64_t end, MfPlan p, const T* __restrict__ vals,
                                                           T* U, int64_t ldu, T* M, int64_t ldm, int64_t m, int64_t n,
                                                           int64_t nnz, int f, T lr, T* abs_err) {
  const int64_t pos = begin + ((int64_t)blockIdx.x * MF_BLOCK + threadIdx.x) / L;
  if (pos < end) mf_rating<T, L, K>(pos, threadIdx.x % L, p, vals, U, ldu, M, ldm, m, n, nnz, f, lr, abs_err);   // (whole ratings: L divides 64)
}

// the levels lv0 .. lv1 - 1, one workgroup: what a level wrote is read by the next one behind the barrier (the
// workgroup's waves share their compute unit's L1; __syncthreads() waits for the stores)
template <typename T, int L, int K>
__global__ __launch_bounds__(MF_BLOCK) void mf_narrow_kernel(int lv0, int lv1, MfPlan p, const T* __restrict__ vals, T* U,
                                                             int64_t ldu, T* M, int64_t ldm, int64_t m, int64_t n,
                                                             int64_t nnz, int f, T lr, T* abs_err) {
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  for (int lv = lv0; lv < lv1; ++lv) {
    const int64_t begin = p.level_off[lv], end = p.level_off[lv + 1];
    for (int64_t pos = begin + g; pos < end; pos += MF_BLOCK / L)
      mf_rating<T, L, K>(pos, l, p, vals, U, ldu, M, ldm, m, n, nnz, f, lr, abs_err);
    __syncthreads();
  }
}

// ---- the plan --------------------------------------------------------------------------------------------------------
constexpr int MF_HEAD = 16;          // int64 words

inline size_t mf_align8(size_t b) { return (b + 7) & ~(size_t)7; }

// the five arrays of the plan at `base` (NULL: nothing is read); false where the head is not this tile's
bool mf_plan_views(const void* h_plan, const void* base, int64_t m, int64_t n, int64_t nnz, MfPlan* out, int64_t* levels,
                   int64_t* segments) {
  const int64_t* h = (const int64_t*)h_plan;
  if (!h || h[0] != SP_MF_PLAN_MAGIC || h[1] != m || h[2] != n || h[3] != nnz) return false;
  const int64_t lv = h[4], sg = h[5], used = h[6];
  if (lv < 0 || lv > nnz || sg < 0 || sg > lv || used < (int64_t)(MF_HEAD * 8)) return false;
  const int64_t need[5] = {nnz * 4, nnz * 4, nnz * 4, (lv + 1) * 4, sg * 16};
  for (int a = 0; a < 5; ++a)
    if (h[7 + a] < (int64_t)(MF_HEAD * 8) || (h[7 + a] & 3) || h[7 + a] + need[a] > used) return false;
  const char* b = (const char*)base;
  out->entry = (const int32_t*)(b + h[7]);
  out->row = (const int32_t*)(b + h[8]);
  out->col = (const int32_t*)(b + h[9]);
  out->level_off = (const int32_t*)(b + h[10]);
  out->segment = (const int32_t*)(b + h[11]);
  *levels = lv;
  *segments = sg;
  return true;
}

bool mf_structure_ok(const char* who, int64_t m, int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices) {
  if (indptr[0] != 0 || indptr[m] != nnz) {
    sp_set_error("%s: indptr runs from %lld to %lld for %lld entries", who, (long long)indptr[0], (long long)indptr[m],
                 (long long)nnz);
    return false;
  }
  for (int64_t i = 0; i < m; ++i)
    if (indptr[i + 1] < indptr[i]) {
      sp_set_error("%s: indptr is not monotone at row %lld", who, (long long)i);
      return false;
    }
  for (int64_t e = 0; e < nnz; ++e)
    if (indices[e] < 0 || indices[e] >= n) {
      sp_set_error("%s: index %d of entry %lld is outside 0 .. %lld", who, (int)indices[e], (long long)e, (long long)n - 1);
      return false;
    }
  return true;
}

// ---- the plain loop ----------------------------------------------------------------------------------------------------
template <typename T, int L>
void mf_host_loop(int64_t f, int64_t nnz, const int32_t* rows, const int32_t* cols, const T* vals, T* U, int64_t ldu, T* M,
                  int64_t ldm, T lr, T* abs_err, const int32_t* order) {
  T lane[L];
  for (int64_t t = 0; t < nnz; ++t) {
    const int64_t e = order ? order[t] : t;
    T* up = U + (int64_t)rows[e] * ldu;
    T* mp = M + (int64_t)cols[e] * ldm;
    for (int l = 0; l < L; ++l) {
      T s = (T)0;
      for (int64_t k = l; k < f; k += L) s = s + up[k] * mp[k];
      lane[l] = s;
    }
    for (int w = L / 2; w >= 1; w >>= 1)
      for (int l = 0; l < w; ++l) lane[l] = lane[l] + lane[l + w];
    const T d = vals[e] - lane[0];
    for (int64_t k = 0; k < f; ++k) {
      up[k] = up[k] + (up[k] * d) * lr;
      mp[k] = mp[k] + (mp[k] * d) * lr;
    }
    if (abs_err) abs_err[e] = std::fabs(d);
  }
}

// what sp_sgd_mf and sp_sgd_mf_host refuse alike
template <typename T>
int mf_check(const char* who, int64_t m, int64_t n, int64_t f, int64_t nnz, int64_t ldu, int64_t ldm, double lr) {
  if (m < 0 || n < 0 || nnz < 0 || m > 0x7fffffffLL || n > 0x7fffffffLL || nnz > 0x7fffffffLL)
    SP_FAIL("%s: bad sizes m=%lld n=%lld nnz=%lld (each 0 .. 2^31 - 1)", who, (long long)m, (long long)n, (long long)nnz);
  if (f < 1 || f > SP_MF_MAX_F) SP_FAIL("%s: f = %lld must be in 1 .. %d", who, (long long)f, SP_MF_MAX_F);
  if (ldu < f || ldm < f)
    SP_FAIL("%s: leading dimensions %lld, %lld below f = %lld", who, (long long)ldu, (long long)ldm, (long long)f);
  if (!std::isfinite(lr) || !std::isfinite((T)lr)) SP_FAIL("%s: lr = %g must be finite", who, lr);
  return 0;
}

template <typename T, int L, int K>
int mf_launch(const MfPlan& dp, const MfPlan& hp, int64_t segments, const T* vals, T* U, int64_t ldu, T* M, int64_t ldm,
              int64_t m, int64_t n, int64_t nnz, int f, T lr, T* abs_err, int64_t* launched, hipStream_t st) {
  for (int64_t s = 0; s < segments; ++s) {
    const int32_t kind = hp.segment[4 * s], lv0 = hp.segment[4 * s + 1], lv1 = hp.segment[4 * s + 2];
    if (kind == SP_MF_SEG_WIDE) {
      const int64_t begin = hp.level_off[lv0], end = hp.level_off[lv0 + 1];
      const int64_t blocks = ((end - begin) * L + MF_BLOCK - 1) / MF_BLOCK;
      hipLaunchKernelGGL((mf_wide_kernel<T, L, K>), dim3((unsigned)blocks), dim3(MF_BLOCK), 0, st, begin, end, dp, vals, U, ldu,
                         M, ldm, m, n, nnz, f, lr, abs_err);
    } else {
      hipLaunchKernelGGL((mf_narrow_kernel<T, L, K>), dim3(1), dim3(MF_BLOCK), 0, st, (int)lv0, (int)lv1, dp, vals, U, ldu, M,
                         ldm, m, n, nnz, f, lr, abs_err);
    }
    SP_CHECK_LAUNCH();
    if (launched) ++*launched;
  }
  return 0;
}

}  // namespace

extern "C" size_t sp_sgd_mf_plan_bytes(int64_t m, int64_t n, int64_t nnz) {
  if (m < 0 || n < 0 || nnz < 0 || m > 0x7fffffffLL || n > 0x7fffffffLL || nnz > 0x7fffffffLL) return 0;
  // entry, row, col, level_off (at most nnz levels), segment (at most one per level), each 8-byte aligned
  return (size_t)MF_HEAD * 8 + 3 * mf_align8((size_t)nnz * 4) + mf_align8((size_t)(nnz + 1) * 4) + (size_t)nnz * 16;
}

extern "C" int sp_sgd_mf_plan(int64_t m, int64_t n, int64_t nnz, const int64_t* h_indptr, const int32_t* h_indices,
                              void* h_plan, size_t bytes) {
  if (m < 0 || n < 0 || nnz < 0) SP_FAIL("sp_sgd_mf_plan: negative size");
  if (m > 0x7fffffffLL || n > 0x7fffffffLL) SP_FAIL("sp_sgd_mf_plan: m and n must be below 2^31");
  if (nnz > 0x7fffffffLL) SP_FAIL("sp_sgd_mf_plan: nnz = %lld must be below 2^31", (long long)nnz);
  if (!h_indptr || !h_plan || (nnz > 0 && !h_indices)) SP_FAIL("sp_sgd_mf_plan: NULL pointer");
  if (bytes < sp_sgd_mf_plan_bytes(m, n, nnz)) SP_FAIL("sp_sgd_mf_plan: %zu bytes for a plan of up to %zu", bytes, sp_sgd_mf_plan_bytes(m, n, nnz));
  if (!mf_structure_ok("sp_sgd_mf_plan", m, n, nnz, h_indptr, h_indices)) return 1;

  // level(e) = 1 + max(level of the previous entry of e's row, of e's column)
  std::vector<int32_t> level((size_t)nnz), rowlast((size_t)m, 0), collast((size_t)n, 0);
  int64_t levels = 0;
  for (int64_t i = 0; i < m; ++i)
    for (int64_t e = h_indptr[i]; e < h_indptr[i + 1]; ++e) {
      const int32_t j = h_indices[e];
      const int32_t lv = 1 + (rowlast[i] > collast[j] ? rowlast[i] : collast[j]);
      level[e] = lv;
      rowlast[i] = collast[j] = lv;
      if (lv > levels) levels = lv;
    }
  // segments: a wide level alone, a maximal run of narrow levels together
  std::vector<int32_t> count((size_t)levels + 1, 0);      // count[v + 1]: entries of level v (0-based), then offsets
  for (int64_t e = 0; e < nnz; ++e) ++count[level[e]];
  int64_t segments = 0;
  for (int64_t v = 0; v < levels; ++v) {
    const bool wide = count[v + 1] >= SP_MF_WIDE;
    if (wide || v == 0 || count[v] >= SP_MF_WIDE) ++segments;
  }
  int64_t* h = (int64_t*)h_plan;
  size_t at = (size_t)MF_HEAD * 8;
  const size_t off_entry = at;
  at += mf_align8((size_t)nnz * 4);
  const size_t off_row = at;
  at += mf_align8((size_t)nnz * 4);
  const size_t off_col = at;
  at += mf_align8((size_t)nnz * 4);
  const size_t off_level = at;
  at += mf_align8((size_t)(levels + 1) * 4);
  const size_t off_seg = at;
  at += (size_t)segments * 16;
  memset(h_plan, 0, at);
  h[0] = SP_MF_PLAN_MAGIC;
  h[1] = m;
  h[2] = n;
  h[3] = nnz;
  h[4] = levels;
  h[5] = segments;
  h[6] = (int64_t)at;
  h[7] = (int64_t)off_entry;
  h[8] = (int64_t)off_row;
  h[9] = (int64_t)off_col;
  h[10] = (int64_t)off_level;
  h[11] = (int64_t)off_seg;
  h[12] = SP_MF_WIDE;
  char* b = (char*)h_plan;
  int32_t *entry = (int32_t*)(b + off_entry), *row = (int32_t*)(b + off_row), *col = (int32_t*)(b + off_col);
  int32_t *level_off = (int32_t*)(b + off_level), *seg = (int32_t*)(b + off_seg);
  int64_t s = 0;
  for (int64_t v = 0; v < levels; ++v) {
    const bool wide = count[v + 1] >= SP_MF_WIDE;
    if (wide || v == 0 || count[v] >= SP_MF_WIDE) {
      seg[4 * s] = wide ? SP_MF_SEG_WIDE : SP_MF_SEG_NARROW;
      seg[4 * s + 1] = (int32_t)v;
      ++s;
    }
    seg[4 * (s - 1) + 2] = (int32_t)(v + 1);
  }
  // counting sort by level, stable: ascending entry index inside a level
  level_off[0] = 0;
  for (int64_t v = 0; v < levels; ++v) level_off[v + 1] = level_off[v] + count[v + 1];
  std::vector<int32_t> next(level_off, level_off + levels);
  for (int64_t i = 0; i < m; ++i)
    for (int64_t e = h_indptr[i]; e < h_indptr[i + 1]; ++e) {
      const int32_t pos = next[level[e] - 1]++;
      entry[pos] = (int32_t)e;
      row[pos] = (int32_t)i;
      col[pos] = h_indices[e];
    }
  return 0;
}

extern "C" int sp_sgd_mf_host(int32_t dtype, int64_t m, int64_t n, int64_t f, int64_t nnz, const int64_t* h_indptr,
                              const int32_t* h_indices, const void* h_vals, void* h_U, int64_t ldu, void* h_M, int64_t ldm,
                              double lr, void* h_abs_err, const int32_t* h_order) {
  return sp_float_dispatch("sp_sgd_mf_host", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (int rc = mf_check<T>("sp_sgd_mf_host", m, n, f, nnz, ldu, ldm, lr)) return rc;
    if (!h_indptr || (nnz > 0 && (!h_indices || !h_vals || !h_U || !h_M))) SP_FAIL("sp_sgd_mf_host: NULL pointer");
    if (!mf_structure_ok("sp_sgd_mf_host", m, n, nnz, h_indptr, h_indices)) return 1;
    if (h_order)
      for (int64_t e = 0; e < nnz; ++e)
        if (h_order[e] < 0 || h_order[e] >= nnz) SP_FAIL("sp_sgd_mf_host: order[%lld] = %d is no entry", (long long)e, (int)h_order[e]);
    if (nnz == 0) return 0;
    std::vector<int32_t> rows((size_t)nnz);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t e = h_indptr[i]; e < h_indptr[i + 1]; ++e) rows[e] = (int32_t)i;
    auto go = [&](auto lanes) {
      mf_host_loop<T, decltype(lanes)::value>(f, nnz, rows.data(), h_indices, (const T*)h_vals, (T*)h_U, ldu, (T*)h_M, ldm,
                                              (T)lr, (T*)h_abs_err, h_order);
      return 0;
    };
    const int L = mf_lanes(f);
    if (L == 8) return go(std::integral_constant<int, 8>());
    if (L == 16) return go(std::integral_constant<int, 16>());
    return go(std::integral_constant<int, 64>());
  });
}

extern "C" int sp_sgd_mf(int32_t dtype, int64_t m, int64_t n, int64_t f, int64_t nnz, const void* d_vals, const void* d_plan,
                         const void* h_plan, void* d_U, int64_t ldu, void* d_M, int64_t ldm, double lr, void* d_abs_err,
                         int64_t* launched, void* stream) {
  if (launched) *launched = 0;
  return sp_float_dispatch("sp_sgd_mf", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (int rc = mf_check<T>("sp_sgd_mf", m, n, f, nnz, ldu, ldm, lr)) return rc;
    if (nnz == 0) return 0;
    if (!d_vals || !d_plan || !h_plan || !d_U || !d_M) SP_FAIL("sp_sgd_mf: vals, the plan (both copies), U and M are required");
    MfPlan hp, dp;
    int64_t levels = 0, segments = 0;
    if (!mf_plan_views(h_plan, h_plan, m, n, nnz, &hp, &levels, &segments) ||
        !mf_plan_views(h_plan, d_plan, m, n, nnz, &dp, &levels, &segments))
      SP_FAIL("sp_sgd_mf: the plan is not one of a %lld x %lld tile with %lld entries", (long long)m, (long long)n,
              (long long)nnz);
    for (int64_t s = 0; s < segments; ++s) {
      const int32_t kind = hp.segment[4 * s], lv0 = hp.segment[4 * s + 1], lv1 = hp.segment[4 * s + 2];
      if ((kind != SP_MF_SEG_WIDE && kind != SP_MF_SEG_NARROW) || lv0 < 0 || lv1 <= lv0 || lv1 > levels ||
          (kind == SP_MF_SEG_WIDE && lv1 != lv0 + 1))
        SP_FAIL("sp_sgd_mf: segment %lld of the plan is malformed", (long long)s);
    }
    for (int64_t v = 0; v < levels; ++v)
      if (hp.level_off[v] < 0 || hp.level_off[v + 1] < hp.level_off[v] || hp.level_off[v + 1] > nnz)
        SP_FAIL("sp_sgd_mf: the plan's level offsets are malformed");
    auto go = [&](auto lanes, auto per_lane) -> int {
      return mf_launch<T, decltype(lanes)::value, decltype(per_lane)::value>(
          dp, hp, segments, (const T*)d_vals, (T*)d_U, ldu, (T*)d_M, ldm, m, n, nnz, (int)f, (T)lr, (T*)d_abs_err, launched,
          (hipStream_t)stream);
    };
    using std::integral_constant;
    const int L = mf_lanes(f);
    if (L == 8) return go(integral_constant<int, 8>(), integral_constant<int, 2>());
    if (L == 16) return go(integral_constant<int, 16>(), integral_constant<int, 4>());
    return go(integral_constant<int, 64>(), integral_constant<int, 8>());
  });
}
