/* C-ABI of the nearest-neighbour kernels in libspartan_hip_extras.so (csrc/knn.hip; `make extras`).  A header of its
 * own, bound as _hip.EXPORTS_KNN: the sets of functions spartan_hip_extras.h and spartan_hip_eig.h declare are fixed,
 * name by name, by tests. */
#ifndef SPARTAN_HIP_KNN_H_
#define SPARTAN_HIP_KNN_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest k sp_knn / sp_knn_merge take (a larger one is refused; a caller that wants more sorts) */
#define SP_KNN_MAX_K 128

/* sp_knn: for every row of Q [nq, d] the k rows of X [np, d] at the smallest squared Euclidean distance, ascending --
 * the per-tile search of the reference's NearestNeighbors (spartan/examples/sklearn/neighbors/unsupervised.py:43-48,
 * there scikit-learn's trees) as one fused pass: distances are never written to HBM and nothing is sorted.
 *   dtype   SP_F32 | SP_F64 (anything else is refused: convert with astype first).
 *   Q, X    row-major, ldq, ldx >= d elements between rows; neither is written.  np <= 2^31 - 2 per call (a tile of a
 *           larger array passes the row at which it begins as index_offset).
 *   k       1 <= k <= SP_KNN_MAX_K.  nq = 0 is accepted; np = 0 yields all padding; d = 0 makes every distance 0.
 *   d_dist2 [nq, k] dense, of `dtype`; d_idx [nq, k] dense int64 = index_offset + row of X.
 * Distance: the DIFFERENCE form in the input precision, d2(q, x) = sum_j (q_j - x_j)^2: one subtract, one multiply and
 * one add per feature, no contraction, the features of a pair added in ascending order j = 0 .. d - 1 onto one
 * accumulator that starts at 0 -- the same for every pair whatever the grid, `splits` or the row's place in a block.
 * (Not |q|^2 + |x|^2 - 2 q.x: its cancellation would make the order of near neighbours depend on where the cloud
 * sits.)  Order of the results: the total order on (d2, index); equal distances go to the lower index, so the output
 * is bit-identical for every value of `splits`.  If fewer than k points qualify (np < k) the trailing slots hold
 * +inf and index -1.  A point whose distance is NaN is never a neighbour; a point at distance +inf is one, after every
 * finite distance.
 *   splits  0: the library chooses; s >= 1: the points are cut into exactly min(s, np) ranges of rows, each searched
 *           by its own workgroups, whose candidate lists go to the workspace and are merged by the code of
 *           sp_knn_merge (nq is often small and np large: this is what fills the device).
 * A workgroup of 256 threads owns 64 queries and streams its range of points through LDS 64 at a time in chunks of 16
 * features, every thread a 4 x 4 block of partial distances; the k candidates of each query live in LDS, sorted; a
 * finished distance is compared with the query's k-th best and only survivors are inserted (by the wave that owns the
 * query, together).  Vector pipe only; no workgroup waits for another.  d_ws: sp_knn_workspace_bytes(...) bytes for
 * the same arguments (0 when nothing is split). */
size_t sp_knn_workspace_bytes(int32_t dtype, int64_t nq, int64_t np, int64_t d, int32_t k, int32_t splits);
int sp_knn(int32_t dtype, const void* d_Q, int64_t ldq, int64_t nq, const void* d_X, int64_t ldx, int64_t np, int64_t d,
           int32_t k, int64_t index_offset, int32_t splits, void* d_dist2, int64_t* d_idx, void* d_ws, size_t ws_bytes,
           void* stream);

/* sp_knn_merge: every row has m candidates (dist2, idx) in any order, row-major with ldc >= m elements between rows
 * in both arrays; entries with idx < 0 are padding and are ignored, and so are entries whose distance is NaN.  Writes
 * the k smallest by (dist2, idx) to d_dist2 / d_idx ([nq, k] dense), padded with +inf / -1 as above.  The inputs are
 * not written and must not overlap the outputs.  Used for the split path inside sp_knn, for the candidates of several
 * tiles of X and for those of several ranks.  One wave per row.  nq = 0 and m = 0 are accepted. */
int sp_knn_merge(int32_t dtype, const void* d_cand_dist2, const int64_t* d_cand_idx, int64_t ldc, int64_t nq, int64_t m,
                 int32_t k, void* d_dist2, int64_t* d_idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_KNN_H_ */
