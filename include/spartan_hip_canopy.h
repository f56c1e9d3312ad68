/* C-ABI of the canopy clustering kernels in libspartan_hip_extras.so (csrc/canopy.hip; `make extras`).  A header of its
 * own, bound as _hip.EXPORTS_CANOPY: the sets of functions the other headers declare are fixed, name by name, by
 * tests. */
#ifndef SPARTAN_HIP_CANOPY_H_
#define SPARTAN_HIP_CANOPY_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sp_canopy: the tile body of the reference's canopy clustering (spartan/examples/canopy_clustering.py:33-65,
 * _canopy_mapper, without its `count > cf` filter) on a row tile X [n, d]: the greedy pass over the rows in order.
 *   dtype   SP_F32 | SP_F64 for X and d_centers alike (anything else is refused: convert with astype first).  All
 *           arithmetic is done in it, call it T.  t1 and t2 are rounded once: T(t1), T(t2).
 *   X       row-major, ldx >= d elements between rows; not written.
 *   chains  >= 1: chain c owns the rows floor(c n / chains) .. floor((c + 1) n / chains) - 1 (sp_svm_dca's cut).  The
 *           chains are independent: each runs the whole loop on its own rows with its own list of canopies.
 *   cap     >= 1: the most canopies a chain may make.  Chain c writes its canopies, in creation order, to the slots
 *           c * cap, c * cap + 1, ... of
 *             d_centers [chains * cap, d], ldc >= d elements between rows: the means, sum / T(count), one IEEE division
 *             d_counts  [chains * cap] int64: the rows the canopy observed, its creating row included
 *             d_rows    [chains * cap] int64: the index in X of its creating row
 *           and their number to d_num [chains] int64.  A chain that would need more than cap canopies stops and
 *           writes d_num[c] = -1; its slots are then unspecified.  cap = the chain's rows always suffices.
 *   d_ws    sp_canopy_workspace_bytes(dtype, n, d, chains, cap) bytes: the creating rows of every chain's canopies,
 *           [chains * cap, d] contiguous.
 * A chain.  For the rows i of the chain ascending, with the canopies made so far in creation order:
 *     d2  = the squared distance of row i and the canopy's CREATING row: one accumulator that starts at 0 and takes
 *           (x_ij - c_j) * (x_ij - c_j) for j = 0, 1, ... in turn -- subtract, multiply, add, each rounded once in T, no
 *           contraction (sp_knn's difference form; the reference's (c - x)^2 has the same bits)
 *     d2 < T(t1), strict: the canopy observes the row: count += 1, sum = sum + x_i (one add per feature)
 *     d2 < T(t2), strict, for any canopy: the row is strongly bound
 *     a row that is not strongly bound becomes a new canopy: creating row i, count = 1, sum = x_i.  The distance of a
 *     row to itself is never taken; a later duplicate of a creating row is observed like any other row.
 * A canopy's sum therefore starts as its creating row and takes the observed rows in ascending row order.  A NaN
 * distance makes both comparisons false: a row with a NaN becomes a canopy of its own that observes nothing else.
 * T(count) is one conversion: exact in fp64, in fp32 exact up to 2^24 and rounded once (to nearest even) above.
 * The result is exactly this sequential loop's, whatever the blocking below.  A chain's bytes depend on its rows, d and
 * the thresholds alone: `chains` calls on the bands give the bytes of one call.  No atomics on global memory; a call
 * repeated on the same operands gives the same bytes.  The `count > cf` filter belongs to the caller.
 * Refused, with nothing launched: a dtype other than the two, negative n, d < 1, ldx < d, ldc < d, chains < 1 or
 * cap < 1 (or so many that chains * n, chains * cap * ldc or the grid overflow), a t1 or t2 that is not finite in T,
 * NULL d_centers, d_counts, d_rows, d_num or d_ws, NULL d_X with n > 0, ws_bytes below the query's answer.  n = 0 is
 * accepted; a chain without rows gives d_num = 0.
 * Kernel (vector pipe only; one launch; no workgroup waits for another):
 *   canopy_kernel  a workgroup of 256 threads per chain.  The chain's rows are taken in blocks of 64.  Per block: the
 *                  64 x 64 distance tiles (sp_d2_tile) of the block against the creating rows in the workspace give,
 *                  through order-free LDS bit operations, the block's `bound` bits and a 64-bit mask of observed rows
 *                  per canopy, and a thread per (canopy, feature) adds the masked rows to the sum in ascending order;
 *                  the tile of the block against itself gives per row the earlier rows within t2 and per row the later
 *                  rows within t1; one wave resolves the block in order -- 64 steps of scalar bit arithmetic: row i is
 *                  new unless it is bound or an earlier NEW row is within t2 -- and the new canopies' creating rows,
 *                  counts and first sums are appended.  The sums live in d_centers, read and written by this workgroup
 *                  alone, and are divided by the counts at the end. */
int sp_canopy(int32_t dtype, const void* d_X, int64_t ldx, int64_t n, int64_t d, double t1, double t2, int64_t chains,
              int64_t cap, void* d_centers, int64_t ldc, int64_t* d_counts, int64_t* d_rows, int64_t* d_num, void* d_ws,
              size_t ws_bytes, void* stream);

/* The bytes sp_canopy needs at d_ws; 0 for arguments it refuses. */
size_t sp_canopy_workspace_bytes(int32_t dtype, int64_t n, int64_t d, int64_t chains, int64_t cap);

/* sp_pdf_label: the reference's _cluster_mapper (canopy_clustering.py:68-92; streaming_kmeans.py holds the same
 * function) on a row tile X [n, d] with the centres C [k, d]: labels[i] <- the lowest j at which
 *     pdf_ij = T(1) / (T(1) + d2_ij)        (one add, one IEEE division; d2 as sp_canopy's, centres in the place of
 *                                            the creating rows)
 * is largest.  A NaN pdf never wins; the label is -1 with k = 0 and for a row whose every pdf is NaN.
 * This is NOT an arg-min of d2: 1 + d2 rounds, so distinct distances can give one pdf (d2 = 0 and d2 = 1e-20 both
 * give 1), and the lower index then wins whichever is nearer -- the reference's strict `max < pdf` from -1.
 *   dtype   SP_F32 | SP_F64 for X and C alike.  ldx, ldc >= d elements between rows; neither is written.
 *   labels  [n] int32, contiguous.
 * Centres beyond k and rows beyond n never reach a result; the label of a row depends on that row and C alone.
 * Refused, with nothing launched: a dtype other than the two, negative n or k, k >= 2^31, d < 1, ldx < d, ldc < d, and
 * with n > 0 NULL d_X or labels, with n > 0 and k > 0 NULL d_C.  n = 0 launches nothing.
 * Kernel (vector pipe only; one launch; no atomics):
 *   pdf_label_kernel  a workgroup of 256 threads owns 64 rows and sweeps the centres 64 at a time with sp_d2_tile;
 *                     thread (ty, tx) keeps the best (pdf, j) of rows 4 ty .. 4 ty + 3 over its centres, j ascending,
 *                     and the 16 threads of a row merge theirs by (larger pdf, then lower j). */
int sp_pdf_label(int32_t dtype, const void* d_X, int64_t ldx, int64_t n, const void* d_C, int64_t ldc, int64_t k,
                 int64_t d, int32_t* labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_CANOPY_H_ */
