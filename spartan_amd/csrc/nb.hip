// The tile body of the reference's naive Bayes fit on a row tile, normalisation and label sums fused:
//   spartan/examples/naive_bayes.py   fit (:37-56: df, the rows' root mean squares, data / rms)
//                                     _sum_instance_by_label_mapper (:6-23: one interpreted step per document)
// The contract is in include/spartan_hip_nb.h.  Two kernels, and two more with more than one row range:
//   nb_rms_kernel         4 waves x 16 rows, a wave its 16 rows at once: lane t adds x^2 of the columns t, t + 64, ...,
//                         a butterfly over the 64 lanes per row, r = sqrt(q / d) into the workspace.
//   nb_accumulate_kernel  a workgroup = a panel of P feature columns x a range of row blocks, a thread per column with
//                         its column of the [label_size, P] accumulators in LDS.  No two threads share an LDS word, so
//                         there is no barrier and no atomic.  Rows in batches of 4, a ring of 2, 4 or 12 batches in
//                         flight (rows, labels and r alike) while one is divided and added in row order.
//   sp_partial_sum_kernel the ranges' partial S, added in ascending order (sp_extras_common.hpp).
//   nb_finish_kernel      the ranges' df counts and their first bad rows.
#include <type_traits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_nb.h"

namespace {

constexpr int RB = SP_NB_ROWS;       // rows per block
constexpr int R = SP_NB_BATCH;       // rows of a batch
static_assert(RB == 64 && R == 4, "nb_rms_kernel is written for blocks of 64 rows, 16 to a wave; the batches for 4 rows");

// a wave-uniform value out of lane `k` of a register
__device__ __forceinline__ int lane_value(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ float lane_value(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ double lane_value(double v, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

template <typename T>
__global__ __launch_bounds__(256) void nb_rms_kernel(const T* __restrict__ X, int64_t ldx, int64_t m, int64_t d,
                                                     T* __restrict__ rms) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * RB + wave * 16;
  if (w0 >= m) return;                  // (the same for the whole wave)
  T q[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) q[i] = (T)0;
  for (int64_t c0 = 0; c0 < d; c0 += 64) {
    const int64_t c = c0 + lane;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const T x = (c < d && w0 + i < m) ? X[(w0 + i) * ldx + c] : (T)0;
      q[i] = q[i] + x * x;
    }
  }
  // per row a balanced tree over the 64 lane sums (addition commutes, so every lane holds the same bits); lane i keeps
  // row i's
  T mine = (T)0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) q[i] = q[i] + __shfl_xor(q[i], s);
    if (lane == i) mine = q[i];
  }
  if (lane < 16 && w0 + lane < m) rms[w0 + lane] = sqrt_t(mine / (T)d);
}

// D batches of R rows are in flight per thread: the fewer waves a CU holds (the accumulators' LDS bounds them), the
// more rows each has to keep in flight to cover the memory's latency
template <typename T, int D>
__global__ __launch_bounds__(256) void nb_accumulate_kernel(const T* __restrict__ X, int64_t ldx, int64_t m, int64_t d,
                                                            const int64_t* __restrict__ labels, int64_t L,
                                                            const T* __restrict__ rms, int64_t panels, int64_t ranges,
                                                            T* __restrict__ S, int64_t lds, int64_t s_stride,
                                                            int64_t* __restrict__ df, int64_t* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_smem[];
  T* acc = reinterpret_cast<T*>(nb_smem);        // [L][P]; thread t touches acc[l * P + t] only
  const int t = threadIdx.x, P = blockDim.x, lane = threadIdx.x & 63;
  const int64_t pn = (int64_t)blockIdx.x % panels, g = (int64_t)blockIdx.x / panels;
  const int64_t col = pn * P + t;
  const bool cv = col < d;
  const int64_t nb = (m + RB - 1) / RB;
  const int64_t row_b = (g * nb / ranges) * RB;
  int64_t row_e = ((g + 1) * nb / ranges) * RB;
  if (row_e > m) row_e = m;

  for (int64_t l = 0; l < L; ++l) acc[l * P + t] = (T)0;
  int64_t count = 0, first_bad = 0;

  // a batch in flight: the thread's column of R rows, and in lane k < R of every wave row k's label (-1 out of range,
  // -2 no such row) and r
  T xr[D][R], rv[D];
  int lv[D];
  auto fetch = [&](int b, int64_t r0) {
#pragma unroll
    for (int k = 0; k < R; ++k) xr[b][k] = (cv && r0 + k < row_e) ? X[(r0 + k) * ldx + col] : (T)0;
    const int64_t row = r0 + lane;
    lv[b] = -2;
    rv[b] = (T)1;
    if (lane < R && row < row_e) {
      const int64_t lb = labels[row];
      lv[b] = (lb >= 0 && lb < L) ? (int)lb : -1;
      rv[b] = rms[row];
    }
  };
#pragma unroll
  for (int b = 0; b < D; ++b) fetch(b, row_b + b * R);
  for (int64_t r0 = row_b; r0 < row_e; r0 += D * R) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const int64_t rb0 = r0 + b * R;
      if (rb0 >= row_e) continue;       // (the same for the whole workgroup)
      T z[R], v[R];
      int lab[R];
      int positive = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        lab[k] = lane_value(lv[b], k);
        if (lab[k] == -1 && first_bad == 0) first_bad = rb0 + k + 1;
        z[k] = xr[b][k] / lane_value(rv[b], k);
        positive += (xr[b][k] > (T)0) ? 1 : 0;      // (a column or a row that is not there was loaded as 0)
      }
      count += positive;
      fetch(b, rb0 + D * R);
#pragma unroll
      for (int k = 0; k < R; ++k) v[k] = acc[(lab[k] < 0 ? 0 : lab[k]) * P + t];
      // row order: a later row of this batch with the same label goes on from this row's sum
#pragma unroll
      for (int k = 0; k < R; ++k) {
        v[k] = v[k] + z[k];
#pragma unroll
        for (int k2 = k + 1; k2 < R; ++k2)
          if (lab[k] >= 0 && lab[k2] == lab[k]) v[k2] = v[k];
      }
#pragma unroll
      for (int k = 0; k < R; ++k)
        if (lab[k] >= 0) acc[lab[k] * P + t] = v[k];
    }
  }

  if (cv) {
    T* So = S + g * s_stride;
    for (int64_t l = 0; l < L; ++l) So[l * lds + col] = acc[l * P + t];
    df[g * d + col] = count;
  }
  if (pn == 0 && t == 0) bad[g] = first_bad;
}

// df[j] <- the ranges' counts added; bad <- the lowest row + 1 any range reports (0: none).  A workgroup takes 64
// columns at a time, its four waves every fourth range each (integer sums: any order), so that a thread's loads do not
// wait for one another; no early exit in the search for bad either
__global__ __launch_bounds__(256) void nb_finish_kernel(const int64_t* __restrict__ pdf, const int64_t* __restrict__ pbad,
                                                        int64_t ranges, int64_t d, int64_t* __restrict__ df,
                                                        int64_t* __restrict__ bad) {
  __shared__ int64_t part[256];
  const int tid = threadIdx.x, s = tid >> 6, jl = tid & 63;
  for (int64_t j0 = (int64_t)blockIdx.x * 64; j0 < d; j0 += (int64_t)gridDim.x * 64) {
    const int64_t j = j0 + jl;
    int64_t a = 0;
    if (j < d) {
#pragma unroll 8
      for (int64_t g = s; g < ranges; g += 4) a += pdf[g * d + j];
    }
    part[tid] = a;
    __syncthreads();
    if (s == 0 && j < d) df[j] = part[jl] + part[64 + jl] + part[128 + jl] + part[192 + jl];
    __syncthreads();
  }
  if (blockIdx.x == 0) {
    const int64_t none = 0x7fffffffffffffffLL;
    int64_t low = none;
#pragma unroll 4
    for (int64_t g = tid; g < ranges; g += 256) {
      const int64_t v = pbad[g];
      if (v != 0 && v < low) low = v;
    }
    part[tid] = low;
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < 256; ++i)
        if (part[i] < low) low = part[i];
      bad[0] = low == none ? 0 : low;
    }
  }
}

// the threads of a workgroup of the accumulation = the feature columns of its panel
int nb_panel(size_t sz, int64_t L, int64_t d) {
  int p = 256;
  while (p > 64 && ((size_t)L * p * sz > SP_NB_LDS_BYTES || p / 2 >= d)) p /= 2;
  return p;
}
int64_t nb_panels(int p, int64_t d) { return d > 0 ? (d + p - 1) / p : 1; }      // (d = 0: one panel, for bad)

// the workgroups of the accumulation a CU holds at once: its 160 KiB of LDS and its 32 waves bound them
int64_t nb_per_cu(size_t sz, int64_t L, int p) {
  int64_t per_cu = (int64_t)(160 * 1024 / ((size_t)L * p * sz));
  if (per_cu > 2048 / p) per_cu = 2048 / p;
  return per_cu;
}

// the number of ranges the row blocks are cut into
int64_t nb_ranges(size_t sz, int64_t m, int64_t d, int64_t L, int32_t splits) {
  const int64_t nb = (m + RB - 1) / RB;
  if (nb <= 1) return 1;
  if (splits >= 1) return splits < nb ? splits : nb;
  // the library's choice: as many workgroups as the CUs hold at once, every range at least eight row blocks long so
  // that the partials (ranges x label_size x d) stay small beside the rows read
  const int p = nb_panel(sz, L, d);
  const int64_t per_cu = nb_per_cu(sz, L, p);
  const int64_t panels = nb_panels(p, d);
  int64_t want = (SP_CUS * per_cu + panels - 1) / panels;
  if (want > nb / 8) want = nb / 8;
  if (want > 512) want = 512;
  return want < 1 ? 1 : want;
}

// the workspace: r (a value per row), then with more than one range their partial sums, counts and first bad rows
struct Layout {
  int64_t ranges;
  size_t r_bytes, s_bytes, df_bytes, bad_bytes;
  size_t total() const { return r_bytes + s_bytes + df_bytes + bad_bytes; }
};

Layout nb_layout(size_t sz, int64_t m, int64_t d, int64_t L, int32_t splits) {
  Layout l;
  l.ranges = nb_ranges(sz, m, d, L, splits);
  l.r_bytes = sp_align256((size_t)(m > 0 ? m : 1) * sz);
  l.s_bytes = l.ranges > 1 ? sp_align256((size_t)l.ranges * L * d * sz) : 0;
  l.df_bytes = l.ranges > 1 ? sp_align256((size_t)l.ranges * d * sizeof(int64_t)) : 0;
  l.bad_bytes = l.ranges > 1 ? (size_t)l.ranges * sizeof(int64_t) : 0;
  return l;
}

bool nb_shape_ok(int64_t m, int64_t d, int64_t L, int32_t splits) {
  return m >= 0 && d >= 0 && L >= 1 && L <= SP_NB_MAX_LABELS && splits >= 0;
}

template <typename T>
int nb_run(const T* X, int64_t ldx, int64_t m, int64_t d, const int64_t* labels, int64_t L, int32_t splits, T* S,
           int64_t lds, int64_t* df, int64_t* bad, void* ws, size_t ws_bytes, hipStream_t st) {
  const Layout l = nb_layout(sizeof(T), m, d, L, splits);
  const int p = nb_panel(sizeof(T), L, d);
  const int64_t ranges = l.ranges, panels = nb_panels(p, d), nb = (m + RB - 1) / RB;
  if (!ws || ws_bytes < l.total()) SP_FAIL("sp_nb_step: workspace of %zu bytes, %zu needed", ws_bytes, l.total());
  if (nb > 0x7fffffffLL || (double)panels * (double)ranges > 2147483647.0)
    SP_FAIL("sp_nb_step: m=%lld d=%lld are too many workgroups for one launch", (long long)m, (long long)d);
  unsigned char* wsb = reinterpret_cast<unsigned char*>(ws);
  T* rms = reinterpret_cast<T*>(wsb);
  T* ps = reinterpret_cast<T*>(wsb + l.r_bytes);
  int64_t* pdf = reinterpret_cast<int64_t*>(wsb + l.r_bytes + l.s_bytes);
  int64_t* pbad = reinterpret_cast<int64_t*>(wsb + l.r_bytes + l.s_bytes + l.df_bytes);

  if (m > 0 && d > 0) {
    hipLaunchKernelGGL(nb_rms_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, X, ldx, m, d, rms);
    SP_CHECK_LAUNCH();
  }
  const size_t smem = (size_t)L * p * sizeof(T);
  // rows in flight per thread: 48, 16 or 8 as a CU holds up to 8, up to 16 or more waves of this kernel
  const int64_t waves = nb_per_cu(sizeof(T), L, p) * (p / 64);
  auto launch = [&](auto depth) -> int {
    constexpr int D = decltype(depth)::value;
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(nb_accumulate_kernel<T, D>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, SP_NB_LDS_BYTES));
    if (ranges > 1)
      hipLaunchKernelGGL((nb_accumulate_kernel<T, D>), dim3((unsigned)(panels * ranges)), dim3(p), smem, st, X, ldx, m, d,
                         labels, L, rms, panels, ranges, ps, d, L * d, pdf, pbad);
    else
      hipLaunchKernelGGL((nb_accumulate_kernel<T, D>), dim3((unsigned)panels), dim3(p), smem, st, X, ldx, m, d, labels, L,
                         rms, panels, (int64_t)1, S, lds, (int64_t)0, df, bad);
    SP_CHECK_LAUNCH();
    return 0;
  };
  if (waves <= 8 ? launch(std::integral_constant<int, 12>()) : waves <= 16 ? launch(std::integral_constant<int, 4>())
                                                                           : launch(std::integral_constant<int, 2>()))
    return 1;
  if (ranges > 1) {
    // S[l, j] <- P_0[l, j] + P_1[l, j] + ... in ascending order
    if (sp_partial_sum<T>(ps, ranges, L, d, S, lds, (const T*)nullptr, 0, (T*)nullptr, st)) return 1;
    int64_t blocks = (d + 63) / 64;
    if (blocks < 1) blocks = 1;
    if (blocks > SP_CUS * SP_BLOCKS_PER_CU) blocks = SP_CUS * SP_BLOCKS_PER_CU;
    hipLaunchKernelGGL(nb_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pdf, pbad, ranges, d, df, bad);
    SP_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" size_t sp_nb_step_workspace_bytes(int32_t dtype, int64_t m, int64_t d, int64_t label_size, int32_t splits) {
  if ((dtype != SP_F32 && dtype != SP_F64) || !nb_shape_ok(m, d, label_size, splits)) return 0;
  return nb_layout(sp_dtype_size(dtype), m, d, label_size, splits).total();
}

extern "C" int sp_nb_step(int32_t dtype, const void* d_X, int64_t ldx, int64_t m, int64_t d, const int64_t* d_labels,
                          int64_t label_size, int32_t splits, void* d_S, int64_t lds, int64_t* d_df, int64_t* d_bad,
                          void* d_ws, size_t ws_bytes, void* stream) {
  return sp_float_dispatch("sp_nb_step", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (label_size < 1 || label_size > SP_NB_MAX_LABELS)
      SP_FAIL("sp_nb_step: label_size = %lld must be in 1 .. %d", (long long)label_size, SP_NB_MAX_LABELS);
    if (!nb_shape_ok(m, d, label_size, splits) || ldx < d || lds < d)
      SP_FAIL("sp_nb_step: bad shape m=%lld d=%lld ldx=%lld lds=%lld splits=%d", (long long)m, (long long)d,
              (long long)ldx, (long long)lds, (int)splits);
    if (!d_bad || (d > 0 && (!d_S || !d_df))) SP_FAIL("sp_nb_step: S, df and bad are required");
    if (m > 0 && (!d_labels || (d > 0 && !d_X))) SP_FAIL("sp_nb_step: X and labels are required");
    return nb_run<T>((const T*)d_X, ldx, m, d, d_labels, label_size, splits, (T*)d_S, lds, d_df, d_bad, d_ws, ws_bytes,
                     (hipStream_t)stream);
  });
}
