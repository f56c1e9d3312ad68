/* C-ABI of the LIBOR-market-model swaption path kernel in libspartan_hip_extras.so (csrc/lmm.hip; `make extras`).  A
 * header of its own, bound as _hip.EXPORTS_LMM: the sets of functions the other headers declare are fixed, name by
 * name, by tests. */
#ifndef SPARTAN_HIP_LMM_H_
#define SPARTAN_HIP_LMM_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the most maturities of a product: a workgroup of 64 pairs keeps K values per pair in LDS, 128 * 64 doubles = 64 KiB */
#define SP_LMM_MAX_K 128

/* sp_lmm_swaption: the discounted payoff of one European payer swaption under Andersen's LIBOR market model
 * (spartan/examples/swaption.py:47-97, one product of `simulate`) for n antithetic pairs of paths: every pair walks
 * K = `maturities` forward rates through S = `steps` time steps with the draws of its column, once with the draws as
 * they are and once negated, and the two discounted payoffs are averaged.
 *   dtype   SP_F32 | SP_F64 for the draws and the output alike (anything else is refused: convert with astype first).
 *           All arithmetic is done in it, call it T.
 *   d_eps   [steps, n] draws, ld_eps >= n elements between rows (a band of columns of a wider array is taken as it
 *           is); not written.
 *   d_out   [n], contiguous, written whole.
 *   steps, maturities   1 <= S < K <= SP_LMM_MAX_K.
 *   lamb, delta, f0, theta   the volatility, the accrual period, the flat initial forward rate and the strike; each is
 *           rounded once, lam = T(lamb), D = T(delta), F = T(f0), TH = T(theta).
 * Arithmetic.  Every operation is rounded once in T, no contraction, IEEE division and square root.  The constants
 *     c0 = ((T(0.5) * lam) * lam) * D      sq = sqrt(D)      cth = TH * D
 * are formed once on the host.  For pair p and sign s = +1, then s = -1:
 *     f[0..K-1] = F;  b = 1
 *     for t = 1 .. S:
 *         b = b * (1 + D * f[t-1])
 *         z = (lam * (s * eps[t-1, p])) * sq
 *         mu = 0
 *         for k = t .. K-1:                        (ascending; f[k] is read before it is replaced)
 *             df = D * f[k]
 *             mu = mu + (lam * df) / (1 + df)
 *             f[k] = f[k] * exp(((lam * mu) * D - c0) + z)
 *     zc = 1;  acc = 0
 *     for k = S .. K-1:
 *         zc = zc / (1 + D * f[k])
 *         acc = acc + zc
 *     x = (1 - zc) - cth * acc
 *     v_s = (x < 0 ? 0 : x) / b                    (numpy.maximum(x, 0): a NaN stays NaN; not fmax)
 *     out[p] = (v_+ + v_-) / 2
 * exp is the device library's: expf for float (the compiler's accurate expansion of its exp builtin -- no fast-math
 * flag is given and denormals are kept) and exp for double (__ocml_exp_f64).  HIP's documentation of its device math
 * functions gives both a maximum error of 1 ulp; the tests' bound takes 2 ulp for exp of a perturbed argument, the
 * figure the project takes for pow.  Everything else in the recurrence is an IEEE operation, so exp alone separates
 * the kernel from NumPy.
 * The bits of out[p] depend on column p of eps and the scalars alone: not on n, on ld_eps, or on the lane or workgroup
 * the pair lands in.  A band of pairs computed alone gives the bits the whole gives; a repeated call gives the same
 * bits.  No atomics, no workspace.  A NaN or an infinity among the draws stays in its own pair.
 * Refused, with nothing launched: a dtype other than the two, negative n, ld_eps < n, S or K outside
 * 1 <= S < K <= SP_LMM_MAX_K, a lamb, delta, f0 or theta that is not finite in T, delta <= 0 (in T as well), and with
 * n > 0 a NULL d_eps or d_out.  n = 0 launches nothing.
 * Kernel (vector pipe only; one launch):
 *   lmm_swaption_kernel   one lane per pair, 64 pairs (one wave) to a workgroup, ceil(n / 64) workgroups.  The two
 *                   signs run one after the other through the same state.  f lives in LDS as [k][lane], K * 64 values
 *                   of dynamic LDS per workgroup (10 KiB in float, 20 KiB in double at the reference's K = 40; 64 KiB
 *                   at K = 128 in double), every lane reading and writing its own column only: a wave's accesses are
 *                   64 consecutive words, there is no barrier, and no lane waits for another.  eps[t-1, p] is one
 *                   coalesced row read per step and sign.  The k loop is unrolled by 4: the divisions and exps of four
 *                   maturities are independent, only the additions into mu are a chain. */
int sp_lmm_swaption(int32_t dtype, const void* d_eps, int64_t ld_eps, int64_t n, int32_t steps, int32_t maturities,
                    double lamb, double delta, double f0, double theta, void* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_LMM_H_ */
