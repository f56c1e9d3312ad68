// The tile body of the reference's DisDCA linear SVM on a row tile, one pass of dual coordinate ascent per chain:
//   spartan/examples/disdca_svm.py   _svm_disdca_train (:5-25: two inner products, a division, a clamp and a rank-one
//                                    update of w per row, every row from the w the row before it left)
// The contract is in include/spartan_hip_svm.h.  One kernel:
//   svm_dca_kernel   a wave per chain, 4 chains to a workgroup (2 where w is in LDS); lane l keeps the columns l,
//                    l + 64, ... of w for the whole chain.  No wave shares a word with another: no barrier, no atomic.
//                    Rows in batches of R, a ring of two batches in flight (the lane's columns, and in lanes < R the
//                    rows' y and alpha) while one is worked through in row order.
#include <cmath>
#include <type_traits>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_svm.h"

namespace {

// a wave-uniform value out of lane `k` of a register (as nb.hip's)
__device__ __forceinline__ float svm_lane_value(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ double svm_lane_value(double v, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// the 64 lane sums as a balanced tree, partners at distance 32 first (addition commutes: every lane ends with the
// same bits)
template <typename T>
__device__ __forceinline__ T svm_tree(T p) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s);
  return p;
}

// K values of w per lane (the columns lane, lane + 64, ...), R rows to a batch, D batches in the ring; WL: w lives in
// the wave's K * 64 words of LDS (a lane reads the words it wrote itself and no others), otherwise in registers.
// XR: the ring holds the rows; without it (64 doubles per lane do not fit beside their addresses) only y and alpha
// travel through the ring and a row is read where it is used, for the products and again for the update -- the second
// time out of the caches, and the CU's other waves cover the wait.
template <typename T, int K, int R, int D, bool WL, bool XR>
__global__ __launch_bounds__(WL ? 128 : 256) void svm_dca_kernel(const T* __restrict__ X, int64_t ldx, int64_t m, int64_t d,
                                                                  const T* __restrict__ y, const T* alpha,
                                                                  const T* __restrict__ w0, T s, int64_t chains,
                                                                  T* alpha_out, T* __restrict__ w_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char svm_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (c >= chains) return;              // (the same for the whole wave)
  const int64_t row_b = c * m / chains, row_e = (c + 1) * m / chains;
  T* wl = reinterpret_cast<T*>(svm_smem) + (size_t)wave * K * 64 + lane;      // this lane's column of LDS
  T wr[WL ? 1 : K];

#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int64_t col = (int64_t)k * 64 + lane;
    const T v = col < d ? w0[col] : (T)0;
    if (WL) wl[k * 64] = v;
    else wr[k] = v;
  }

  // a batch in flight: the lane's columns of R rows (0 where there is no row or no column), and in lane r < R row r's
  // label and alpha
  T xr[XR ? D : 1][XR ? R : 1][XR ? K : 1], yv[D], av[D];
  auto fetch = [&](int b, int64_t r0) {
    if (XR) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int64_t col = (int64_t)k * 64 + lane;
          xr[XR ? b : 0][XR ? r : 0][XR ? k : 0] = (r0 + r < row_e && col < d) ? X[(r0 + r) * ldx + col] : (T)0;
        }
    }
    yv[b] = (T)0;
    av[b] = (T)0;
    if (lane < R && r0 + lane < row_e) {
      yv[b] = y[r0 + lane];
      av[b] = alpha[r0 + lane];
    }
  };
  // column k of row r of batch b, which starts at row rb0 (XR: rb0 is the ring's business)
  auto xv = [&](int b, int64_t rb0, int r, int k) -> T {
    if (XR) return xr[XR ? b : 0][XR ? r : 0][XR ? k : 0];
    const int64_t col = (int64_t)k * 64 + lane;
    return col < d ? X[(rb0 + r) * ldx + col] : (T)0;
  };
#pragma unroll
  for (int b = 0; b < D; ++b) fetch(b, row_b + b * R);
  for (int64_t r0 = row_b; r0 < row_e; r0 += D * R) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const int64_t rb0 = r0 + b * R;
      if (rb0 >= row_e) continue;       // (the same for the whole wave)
      // A of the batch's rows: nothing here waits for w
      T A[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        T p = (T)0;
        if (rb0 + r < row_e) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const T x = xv(b, rb0, r, k);
            p = p + x * x;
          }
        }
        A[r] = s * svm_tree(p);
      }
      T mine = (T)0;                    // lane r: row r's new alpha
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (rb0 + r >= row_e) continue;
        const T yi = svm_lane_value(yv[b], r), ai = svm_lane_value(av[b], r);
        T p = (T)0;
#pragma unroll
        for (int k = 0; k < K; ++k) p = p + xv(b, rb0, r, k) * (WL ? wl[k * 64] : wr[WL ? 0 : k]);
        const T B = svm_tree(p);
        const T t = yi - B;
        const T g = t / A[r];
        const T v = yi * (g + ai);
        const T c1 = (v < (T)1) ? v : (T)1;
        const T c2 = (c1 > (T)0) ? c1 : (T)0;
        const T dl = yi * c2 - ai;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          // (a column that is not there stays 0 whatever dl is: 0 * inf would be NaN)
          if ((int64_t)k * 64 + lane < d) {
            const T u = (xv(b, rb0, r, k) * s) * dl;
            if (WL) wl[k * 64] = wl[k * 64] + u;
            else wr[WL ? 0 : k] = wr[WL ? 0 : k] + u;
          }
        }
        if (lane == r) mine = ai + dl;
      }
      if (lane < R && rb0 + lane < row_e) alpha_out[rb0 + lane] = mine;
      fetch(b, rb0 + D * R);
    }
  }

  if (w_out) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t col = (int64_t)k * 64 + lane;
      if (col < d) w_out[c * d + col] = WL ? wl[k * 64] : wr[WL ? 0 : k];
    }
  }
}

template <typename T, int K, int R, bool WL>
int svm_launch(const T* X, int64_t ldx, int64_t m, int64_t d, const T* y, const T* alpha, const T* w0, T s, int64_t chains,
               T* alpha_out, T* w_out, hipStream_t st) {
  constexpr int WAVES = WL ? 2 : 4;
  constexpr bool XR = K * sizeof(T) <= 256;
  constexpr int D = 2;
  const size_t smem = WL ? (size_t)WAVES * K * 64 * sizeof(T) : 0;
  if (WL)
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(svm_dca_kernel<T, K, R, D, WL, XR>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
  const int64_t blocks = (chains + WAVES - 1) / WAVES;
  hipLaunchKernelGGL((svm_dca_kernel<T, K, R, D, WL, XR>), dim3((unsigned)blocks), dim3(WAVES * 64), smem, st, X, ldx, m, d, y,
                     alpha, w0, s, chains, alpha_out, w_out);
  SP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sp_svm_dca(int32_t dtype, const void* d_X, int64_t ldx, int64_t m, int64_t d, const void* d_y,
                          const void* d_alpha, const void* d_w0, double scaled_lambda, int64_t chains, void* d_alpha_out,
                          void* d_w_out, void* stream) {
  return sp_float_dispatch("sp_svm_dca", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (m < 0 || d < 1 || d > SP_SVM_MAX_D || ldx < d)
      SP_FAIL("sp_svm_dca: bad shape m=%lld d=%lld (1 .. %d) ldx=%lld", (long long)m, (long long)d, SP_SVM_MAX_D,
              (long long)ldx);
    if (chains < 1 || (chains + 3) / 4 > 0x7fffffffLL || (double)chains * (double)(m > 0 ? m : 1) > 4.0e18)
      SP_FAIL("sp_svm_dca: chains = %lld must be at least 1 (and chains * m below 4e18)", (long long)chains);
    const T s = (T)scaled_lambda;
    if (!(scaled_lambda > 0.0) || !std::isfinite(scaled_lambda) || !(s > (T)0) || !std::isfinite(s))
      SP_FAIL("sp_svm_dca: scaled_lambda = %g must be finite and > 0", scaled_lambda);
    if (!d_w0 || (m > 0 && (!d_X || !d_y || !d_alpha || !d_alpha_out)))
      SP_FAIL("sp_svm_dca: X, y, alpha, w0 and alpha_out are required");
    if (m == 0 && !d_w_out) return 0;
    const int64_t kn = (d + 63) / 64;
    auto go = [&](auto k, auto r, auto wl) -> int {
      return svm_launch<T, decltype(k)::value, decltype(r)::value, decltype(wl)::value>(
          (const T*)d_X, ldx, m, d, (const T*)d_y, (const T*)d_alpha, (const T*)d_w0, s, chains, (T*)d_alpha_out,
          (T*)d_w_out, (hipStream_t)stream);
    };
    using std::integral_constant;
    using reg = std::false_type;
    using lds = std::true_type;
    if (kn <= 1) return go(integral_constant<int, 1>(), integral_constant<int, 8>(), reg());
    if (kn <= 2) return go(integral_constant<int, 2>(), integral_constant<int, 8>(), reg());
    if (kn <= 4) return go(integral_constant<int, 4>(), integral_constant<int, 4>(), reg());
    if (kn <= 8) return go(integral_constant<int, 8>(), integral_constant<int, 2>(), reg());
    if (kn <= 16) return go(integral_constant<int, 16>(), integral_constant<int, 1>(), reg());
    if (kn <= 32) return go(integral_constant<int, 32>(), integral_constant<int, 1>(), lds());
    return go(integral_constant<int, 64>(), integral_constant<int, 1>(), lds());
  });
}
