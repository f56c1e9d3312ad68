/* C-ABI of the naive Bayes step kernel in libspartan_hip_extras.so (csrc/nb.hip; `make extras`).  A header of its own,
 * bound as _hip.EXPORTS_NB: the sets of functions the other headers declare are fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_NB_H_
#define SPARTAN_HIP_NB_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* rows of X in a block (the unit in which `splits` cuts the rows), the largest number of labels, the rows of a batch
 * of the accumulation, and the most LDS a workgroup's accumulators take */
#define SP_NB_ROWS 64
#define SP_NB_MAX_LABELS 128
#define SP_NB_BATCH 4
#define SP_NB_LDS_BYTES 65536

/* sp_nb_step: the tile body of the reference's naive Bayes fit (spartan/examples/naive_bayes.py:6-23, 37-56) on one
 * row tile X [m, d] of documents x terms with labels [m]:
 *     q_i  = sum_j x_ij^2          r_i = sqrt(q_i / d)          z_ij = x_ij / r_i
 *     S_lj = sum over the rows i with labels_i == l of z_ij                       [label_size, d] in T
 *     df_j = the number of rows i with x_ij > 0  (a NaN is not > 0)               [d] int64, exact
 *     bad  = 0, or 1 + the lowest row whose label is outside 0 .. label_size - 1  int64 [1]
 * The reference multiplies z by idf_j = log(n / (df_j + 1)) + 1 before it sums.  idf is constant over a column, so it
 * factors out of the sum over documents; the kernel leaves it out (the caller multiplies S by it afterwards: another
 * rounding, the same mathematics), which lets df -- which idf needs from EVERY tile -- and S come from one call.
 * Nothing of size m x d is stored: X is read twice, r (m values) passes through the workspace.
 *   dtype   SP_F32 | SP_F64 for X and S alike (anything else is refused: convert with astype first).  All arithmetic is
 *           done in it, call it T; T(d) is rounded once.  Division and sqrt are IEEE.
 *   X       row-major, ldx >= d elements between rows; not written.  d_labels int64 [m], contiguous; not written.
 *   d_S     [label_size, d] with lds >= d between rows; d_df int64 [d]; d_bad int64 [1].  All three are written whole.
 *   Refused, with nothing launched: label_size outside 1 .. 128 (the accumulators live in LDS), negative m, d or
 *           splits, ldx < d or lds < d ("bad shape"), a NULL d_bad, NULL d_S or d_df with d > 0, NULL d_X (with d > 0)
 *           or d_labels with m > 0 ("required"), a workspace that is NULL or too small.
 * Special values (the reference's arithmetic, kept): a row of zeros has r = 0 and z = 0 / 0 = NaN -- it turns its
 * label's whole row of S into NaN and no other row.  m = 0, d = 0 and a label nobody has give zeros.  A label out of
 * range (NumPy would wrap a negative one and raise on a large one): the row adds nothing to S, still counts in df, and
 * is reported through bad.
 * Order.  q_i: lane t of a wave adds x_ij^2 (a multiply, then an add; no contraction) for j = t, t + 64, ... in
 * ascending order onto 0; the 64 lane sums are added as a balanced tree, pairs at distance 32 first, then 16, 8, 4, 2
 * and 1.  So q_i, r_i and z_i. depend on row i and d alone: not on the row's neighbours, its position, m, the grid or
 * `splits`.  S: the rows are cut into `ranges` ranges of whole blocks of 64 rows, range g = row blocks
 * floor(g nb / ranges) .. floor((g + 1) nb / ranges) - 1 with nb = ceil(m / 64); inside a range every S_lj is ONE
 * accumulator that starts at 0 and takes z_ij of its label's rows in ascending row order.  With one range S is
 * therefore bit for bit what adding the rows z_i. onto zeros in row order gives.  With more, the ranges' partial
 * [label_size, d] results go to the workspace and sp_partial_sum_kernel adds them in ascending range order onto
 * range 0's.  No atomics of any kind; a call repeated on the same operands gives the same bits.
 *   splits  0: the library chooses `ranges` from dtype, m, d and label_size only; s >= 1: exactly min(s, nb) ranges.
 * Kernels (vector pipe only; no workgroup waits for another, and none has a barrier):
 *   nb_rms_kernel         a workgroup of 4 waves owns 64 rows, a wave 16 of them, all 16 at once: r into the workspace.
 *   nb_accumulate_kernel  a workgroup per (panel of P features) x (row range), P = 64, 128 or 256 threads, a thread per
 *                         feature column: its column of the [label_size, P] accumulators in LDS (label_size * P *
 *                         sizeof(T) <= 64 KiB sets P, and P / 2 < d unless P is 64), which no other thread touches.  It
 *                         walks its rows in batches of 4: it divides the 4, reads their 4 accumulators, adds in row
 *                         order (a later row of the same label takes the earlier one's result from a register, not
 *                         from LDS) and writes them back, while a ring of 2, 4 or 12 further batches -- the column's
 *                         entries, and per wave the rows' labels and r in its first lanes -- is in flight: 12 where
 *                         the accumulators leave a CU at most 8 waves of this kernel, 4 up to 16 waves, else 2.  The
 *                         same thread counts x > 0 for df; thread 0 of panel 0 keeps the first label out of range.
 *   sp_partial_sum_kernel, nb_finish_kernel   only with more than one range: S, then df (the ranges' counts added)
 *                         and bad (the first range that reports a row).
 *   d_ws    sp_nb_step_workspace_bytes(...) bytes for the same arguments (never 0 for arguments that are taken). */
size_t sp_nb_step_workspace_bytes(int32_t dtype, int64_t m, int64_t d, int64_t label_size, int32_t splits);
int sp_nb_step(int32_t dtype, const void* d_X, int64_t ldx, int64_t m, int64_t d, const int64_t* d_labels,
               int64_t label_size, int32_t splits, void* d_S, int64_t lds, int64_t* d_df, int64_t* d_bad, void* d_ws,
               size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_NB_H_ */
