/* C-ABI of the linear SVM's dual coordinate ascent kernel in libspartan_hip_extras.so (csrc/svm.hip; `make extras`).  A
 * header of its own, bound as _hip.EXPORTS_SVM: the sets of functions the other headers declare are fixed, name by
 * name, by tests. */
#ifndef SPARTAN_HIP_SVM_H_
#define SPARTAN_HIP_SVM_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the most features of a row: a chain's w stays on chip, d / 64 values per lane */
#define SP_SVM_MAX_D 4096

/* sp_svm_dca: the tile body of the reference's DisDCA linear SVM (spartan/examples/disdca_svm.py:5-25,
 * _svm_disdca_train) on a row tile X [m, d] with labels y [m] and dual variables alpha [m], started from w0 [d]: one
 * pass of dual coordinate ascent over the rows, every row from the w the row before it left.
 *   dtype   SP_F32 | SP_F64 for X, y, alpha, w0 and both outputs alike (anything else is refused: convert with astype
 *           first).  All arithmetic is done in it, call it T.  scaled_lambda is rounded once, s = T(scaled_lambda).
 *   X       row-major, ldx >= d elements between rows; not written.  y, alpha, w0 contiguous; y and w0 are not written.
 *           y holds the labels as values of T; nothing below needs them to be +1 or -1.
 *   chains  >= 1: chain c owns the rows floor(c m / chains) .. floor((c + 1) m / chains) - 1.  The chains are
 *           independent and EVERY chain starts from w = w0 (the reference's tiles, each with its own copy of w).
 *   d_alpha_out  [m], written whole; it may be d_alpha itself.
 *   d_w_out      NULL, or [chains, d] contiguous: row c <- the w chain c ends with (w0 for a chain without rows).
 * A row.  Inside a chain, for i ascending, every operation rounded once in T, no contraction, IEEE division:
 *     q  = dot(x_i, x_i)        A  = s * q
 *     B  = dot(x_i, w)          t  = y_i - B          g = t / A
 *     v  = y_i * (g + a_i)
 *     c1 = (v < 1) ? v : 1      c2 = (c1 > 0) ? c1 : 0         (Python's min(1, v), then max(0, .), as the reference
 *     dl = y_i * c2 - a_i                                        writes them: a NaN in v gives 1)
 *     w_j  = w_j + (x_ij * s) * dl   for every j                (the reference's order: (x * s) * dl, then the add)
 *     a_i' = a_i + dl
 * dot(p, r): lane l of 64 starts at +0 and adds p_j * r_j (a multiply, then an add) for j = l, l + 64, ... in ascending
 * order; the 64 lane sums are added as a balanced tree, partners at distance 32 first, then 16, 8, 4, 2 and 1 (the
 * order of q_i in spartan_hip_nb.h).  So a row's result depends on the row, on the w it meets and on d alone: not on m,
 * the grid or the other chains, and `chains` calls on the bands give the bits of one call with `chains`.  No atomics;
 * a call repeated on the same operands gives the same bits.
 * Special values (the reference's arithmetic, kept): a row of zeros has A = 0, g = +-inf (NaN when y_i = 0 as well),
 * clamps like any other v and leaves w unchanged (0 * dl is added only where dl is finite: dl is, after the clamp,
 * unless alpha or y is not).  A NaN in x_i makes B and v NaN and c2 = 1, so dl = y_i - a_i is finite and w becomes
 * NaN exactly where x_i is NaN; later rows keep running, those with a non-zero in such a column with B = NaN and
 * c2 = 1.  A dl that is NaN (a NaN in y or alpha) turns every component of w where the row is not zero into NaN.
 * -inf clamps to 0, +inf to 1.
 * Refused, with nothing launched: a dtype other than the two, negative m, d outside 1 .. SP_SVM_MAX_D, ldx < d,
 * chains < 1 (or so many that chains * m overflows 63 bits or the grid 31), a scaled_lambda that is not finite and
 * > 0, NULL d_w0, and with m > 0 NULL d_X, d_y, d_alpha or d_alpha_out.  m = 0 without d_w_out launches nothing.
 * Kernel (vector pipe only; one launch; no workgroup waits for another and none has a barrier):
 *   svm_dca_kernel  a wave per chain, 4 chains to a workgroup (2 where w is in LDS).  Lane l owns the columns l,
 *                   l + 64, ... of w for the whole chain: in registers up to d = 1024 (ceil(d / 64) rounded up to 1, 2,
 *                   4, 8 or 16 values per lane), in the wave's own LDS above (32 or 64 per lane).  X is read once, w0
 *                   once per chain.  Rows travel in batches of 8, 8, 4, 2, 1 rows (as the values per lane grow) through
 *                   a ring of two batches -- the lane's columns of each row, and in the first lanes the rows' y and
 *                   alpha -- so that the next batch is in flight while this one is used; the q of a batch's rows do
 *                   not depend on w and are formed ahead of the chain of B, one division and the update.  One
 *                   exception: 64 doubles per lane (double, d > 2048) do not fit the registers twice, so there only y
 *                   and alpha travel through the ring and a row is read where it is used -- for the products and
 *                   again, out of the caches, for the update.  After the tree every lane holds the same B; division,
 *                   clamp and dl are computed by all lanes and nothing is broadcast. */
int sp_svm_dca(int32_t dtype, const void* d_X, int64_t ldx, int64_t m, int64_t d, const void* d_y, const void* d_alpha,
               const void* d_w0, double scaled_lambda, int64_t chains, void* d_alpha_out, void* d_w_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_SVM_H_ */
