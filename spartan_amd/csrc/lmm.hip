// One European payer swaption of the reference's LIBOR-market-model Monte-Carlo pricer, all time steps of a pair of
// antithetic paths in one kernel:
//   spartan/examples/swaption.py   simulate (:47-97: per time step a scan over the maturities, an exp map, a slice and
//                                  an assign on a [maturities, paths] plane; then two loops for bonds and discounting)
// The contract is in include/spartan_hip_lmm.h.  One kernel:
//   lmm_swaption_kernel   a lane per pair, a wave per workgroup; the K forward rates of a pair are column `lane` of the
//                         workgroup's [K][64] LDS array.  No lane reads a word another lane wrote: no barrier, no atomic.
#include <cmath>

#include "sp_extras_common.hpp"
#include "../../include/spartan_hip_lmm.h"

namespace {

__device__ __forceinline__ float exp_t(float a) { return expf(a); }
__device__ __forceinline__ double exp_t(double a) { return exp(a); }

constexpr int LMM_LANES = 64;

template <typename T>
__global__ __launch_bounds__(LMM_LANES) void lmm_swaption_kernel(const T* __restrict__ eps, int64_t ld, int64_t n, int S,
                                                                 int K, T lam, T D, T F, T c0, T sq, T cth,
                                                                 T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lmm_smem[];
  const int64_t p = (int64_t)blockIdx.x * LMM_LANES + threadIdx.x;
  if (p >= n) return;
  T* f = reinterpret_cast<T*>(lmm_smem) + threadIdx.x;          // f[k] of this pair is f[k * LMM_LANES]
  const T one = (T)1;
  T v[2];
#pragma unroll 1
  for (int sign = 0; sign < 2; ++sign) {
    for (int k = 0; k < K; ++k) f[k * LMM_LANES] = F;
    T b = one;
    T e = eps[p];                                               // (S >= 1) the next step's draw, read a step ahead
#pragma unroll 1
    for (int t = 1; t <= S; ++t) {
      b = b * (one + D * f[(t - 1) * LMM_LANES]);
      const T draw = sign ? -e : e;
      if (t < S) e = eps[(int64_t)t * ld + p];
      const T z = (lam * draw) * sq;
      T mu = (T)0;
      int k = t;
      for (; k + 4 <= K; k += 4) {
        T fk[4], term[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fk[i] = f[(k + i) * LMM_LANES];
          const T df = D * fk[i];
          term[i] = (lam * df) / (one + df);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          mu = mu + term[i];
          f[(k + i) * LMM_LANES] = fk[i] * exp_t(((lam * mu) * D - c0) + z);
        }
      }
      for (; k < K; ++k) {
        const T fk = f[k * LMM_LANES];
        const T df = D * fk;
        mu = mu + (lam * df) / (one + df);
        f[k * LMM_LANES] = fk * exp_t(((lam * mu) * D - c0) + z);
      }
    }
    T zc = one, acc = (T)0;
    for (int k = S; k < K; ++k) {
      zc = zc / (one + D * f[k * LMM_LANES]);
      acc = acc + zc;
    }
    const T x = (one - zc) - cth * acc;
    v[sign] = (x < (T)0 ? (T)0 : x) / b;                        // (a NaN is not < 0 and stays)
  }
  out[p] = (v[0] + v[1]) / (T)2;
}

}  // namespace

extern "C" int sp_lmm_swaption(int32_t dtype, const void* d_eps, int64_t ld_eps, int64_t n, int32_t steps,
                               int32_t maturities, double lamb, double delta, double f0, double theta, void* d_out,
                               void* stream) {
  return sp_float_dispatch("sp_lmm_swaption", dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (n < 0 || ld_eps < n || (n + LMM_LANES - 1) / LMM_LANES > 0x7fffffffLL)
      SP_FAIL("sp_lmm_swaption: bad shape n=%lld ld_eps=%lld", (long long)n, (long long)ld_eps);
    if (steps < 1 || maturities <= steps || maturities > SP_LMM_MAX_K)
      SP_FAIL("sp_lmm_swaption: steps = %d and maturities = %d must satisfy 1 <= steps < maturities <= %d", (int)steps,
              (int)maturities, SP_LMM_MAX_K);
    const T lam = (T)lamb, D = (T)delta, F = (T)f0, TH = (T)theta;
    if (!std::isfinite(lam) || !std::isfinite(D) || !std::isfinite(F) || !std::isfinite(TH))
      SP_FAIL("sp_lmm_swaption: lamb = %g, delta = %g, f0 = %g and theta = %g must be finite", lamb, delta, f0, theta);
    if (!(D > (T)0)) SP_FAIL("sp_lmm_swaption: delta = %g must be > 0", delta);
    if (n > 0 && (!d_eps || !d_out)) SP_FAIL("sp_lmm_swaption: eps and out are required");
    if (n == 0) return 0;
    // the constants, each operation rounded once in T (-ffp-contract=off holds for the host as well)
    const T c0 = (((T)0.5 * lam) * lam) * D;
    const T sq = std::sqrt(D);
    const T cth = TH * D;
    const size_t smem = (size_t)maturities * LMM_LANES * sizeof(T);
    SP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lmm_swaption_kernel<T>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    const int64_t blocks = (n + LMM_LANES - 1) / LMM_LANES;
    hipLaunchKernelGGL(lmm_swaption_kernel<T>, dim3((unsigned)blocks), dim3(LMM_LANES), smem, (hipStream_t)stream,
                       (const T*)d_eps, ld_eps, n, (int)steps, (int)maturities, lam, D, F, c0, sq, cth, (T*)d_out);
    SP_CHECK_LAUNCH();
    return 0;
  });
}
