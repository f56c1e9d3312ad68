/* C-ABI of the fuzzy k-means step kernel in libspartan_hip_extras.so (csrc/fuzzy.hip; `make extras`).  A header of its
 * own, bound as _hip.EXPORTS_FUZZY: the sets of functions the other headers declare are fixed, name by name, by
 * tests. */
#ifndef SPARTAN_HIP_FUZZY_H_
#define SPARTAN_HIP_FUZZY_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* rows of X a workgroup owns (the unit in which `splits` cuts the rows), centres per pass, and the width of the
 * feature panel of the accumulation */
#define SP_FUZZY_ROWS 64
#define SP_FUZZY_CENTERS 64
#define SP_FUZZY_PANEL 128

/* sp_fuzzy_step: one iteration of the reference's fuzzy k-means (spartan/examples/fuzzy_kmeans.py:41-62, 83-93) on one
 * row tile X [n, d] against all centres C [k, d], as a fused pass: the [n, k] membership matrix is formed in registers
 * and LDS and reaches HBM only if the caller passes d_U.
 *     dist_ij = sqrt(d2_ij),  dist_ij = 1e-10 where it is 0        p_ij = dist_ij ^ e,  e = 1 / (m - 1)
 *     z_i = sum_j p_ij        u_ij = p_ij / z_i                    labels_i = argmax_j u_ij
 *     w_ij = u_ij ^ m         sums_jf = sum_i w_ij x_if            wsum_j = sum_i w_ij
 * (The reference's memberships GROW with distance, so the label is the farthest centre; this is the reference, not
 * textbook fuzzy c-means.)
 *   dtype   SP_F32 | SP_F64 for X, C, sums, wsum and U alike (anything else is refused: convert with astype first).  All
 *           arithmetic is done in it, call it T.
 *   m       finite and > 1, else refused.  T(m) and e = T(1 / (m - 1)) (the quotient taken in double from the m that
 *           was passed) are each rounded once; so is T(1e-10).
 *   X, C    row-major, ldx, ldc >= d elements between rows; neither is written.  k >= 1.  n = 0 is accepted and gives
 *           sums = 0, wsum = 0; d = 0 makes every distance 0, hence every dist = 1e-10 and u = 1 / k.  n, k and d have
 *           no limit but the index types (a launch holds at most 2^31 - 1 workgroups).  A refusal launches nothing.
 *   d_labels [n] int64 or NULL; d_sums [k, d] with lds >= d between rows; d_wsum [k]; d_U [n, k] with ldu >= k between
 *           rows, or NULL: U is written only when it is passed.
 * Distance: the DIFFERENCE form of sp_knn in T, d2_ij = sum_f (x_if - c_jf)^2: one subtract, one multiply and one add
 * per feature, no contraction, the features added in ascending order f = 0 .. d - 1 onto one accumulator that starts
 * at 0 -- the same for every pair whatever the grid, `splits` or the row's place in a block.  sqrt is IEEE.
 * Power: with m == 2 exactly (the double that was passed) there is no pow anywhere: p = dist, w = u * u.  Otherwise
 * p = pow(dist, e) and w = pow(u, T(m)) with powf / pow of T, the functions of the map kernel's POW opcode.
 * Labels: labels_i is the lowest j at which d2_ij is largest (sqrt, pow and the division by z_i are monotone, so this
 * is an arg-max of u_i.), a NaN d2 counting as the largest value and the first NaN winning (NumPy's argmax).
 * Order of z_i: the centres are taken in blocks of 64, j = 64 b .. 64 b + 63 (a centre beyond k adds +0).  In a block
 * the 16 groups of four consecutive centres are each summed in ascending order onto 0; the 16 group sums g_0 .. g_15
 * are added as a balanced tree, (g_t + g_{t^1}) first, then pairs of those at distance 2, 4 and 8; the blocks' sums are
 * added in ascending order onto a z that starts at 0.  The bits of labels_i, z_i and u_i. therefore depend on row i
 * of X and on C alone: not on the row's neighbours, its position, n or `splits`.
 * Sums: w_ij * x_if is a multiply, then an add; no atomics, and a call repeated on the same operands gives the same
 * bits.  The rows are cut into `ranges` ranges of whole blocks of 64 rows, range g = row blocks
 * floor(g nb / ranges) .. floor((g + 1) nb / ranges) - 1 with nb = ceil(n / 64); inside a range the rows are added in
 * ascending order onto accumulators that start at 0; with more than one range the ranges' partial [k, d] and [k]
 * results go to the workspace and a combine kernel adds them in ascending range order onto range 0's.
 *   splits  0: the library chooses `ranges` from n, k and d only; s >= 1: exactly min(s, nb) ranges (1 when n = 0).
 * Kernels (vector pipe only; no workgroup waits for another):
 *   fuzzy_norm_kernel        a workgroup of 256 threads owns 64 rows and sweeps all centres, 64 at a time through LDS
 *                            in chunks of 16 features, every thread a 4 x 4 block of d2 (sp_knn's tile); writes
 *                            labels and z (workspace), then, if U is wanted, sweeps the centres again and writes p / z.
 *   fuzzy_accumulate_kernel  a workgroup per (64 centres) x (panel of 128 features) x (row range): per block of 64
 *                            rows it recomputes the same d2 tile over ALL d features, puts w and the rows' feature
 *                            panel in LDS and adds w^T . X_panel, a thread 4 centres x 8 features; the panel-0
 *                            workgroups carry wsum.  The distances are thus computed 1 + ceil(d / 128) times per call
 *                            (3 n k d flops each time, beside the 2 n k d of the sums): the price of keeping d unbounded
 *                            with the accumulators in registers.
 *   sp_partial_sum_kernel    only with more than one range.
 *   d_ws    sp_fuzzy_step_workspace_bytes(...) bytes for the same arguments (never 0 for arguments that are taken). */
size_t sp_fuzzy_step_workspace_bytes(int32_t dtype, int64_t n, int64_t k, int64_t d, int32_t splits);
int sp_fuzzy_step(int32_t dtype, const void* d_X, int64_t ldx, int64_t n, const void* d_C, int64_t ldc, int64_t k,
                  int64_t d, double m, int32_t splits, int64_t* d_labels, void* d_sums, int64_t lds, void* d_wsum,
                  void* d_U, int64_t ldu, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_FUZZY_H_ */
