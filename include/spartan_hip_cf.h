/* C-ABI of the item-recommender kernels in libspartan_hip_extras.so (csrc/cf.hip; `make extras`).  A header of its own,
 * bound as _hip.EXPORTS_CF: the sets of functions the other headers declare are fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_CF_H_
#define SPARTAN_HIP_CF_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest k sp_item_topk / sp_item_topk_merge take (a larger one is refused; a caller that wants more sorts) */
#define SP_CF_MAX_K 128

/* sp_item_topk: for every target item (column j of T [users, m]) the k source items (columns i of S [users, ns]) of the
 * largest cosine similarity, best first -- the two shuffles of the reference's ItemBasedRecommender
 * (spartan/examples/cf/item_recommender.py: _similarity_mapper's N x N table and the argpartsort of its rows) as one
 * fused pass: similarities are never written to HBM and nothing is sorted.
 *   dtype   SP_F32 | SP_F64 for every operand (anything else is refused: convert with astype first).
 *   T, S    row-major, ITEMS along the contiguous axis, ldt >= m and lds >= ns elements between the rows (users);
 *           neither is written.  They may be two column ranges of one table, ldt == lds its row stride.
 *           ns <= 2^31 - 2 per call (a column range of a wider table passes its first column as index_offset).
 *   tnorm   [m], snorm [ns]: the items' norms, taken as given (the caller computes them once for the whole table).
 *   k       1 <= k <= SP_CF_MAX_K.  m = 0 launches nothing; ns = 0 yields all padding; users = 0 makes every dot +0.
 *   d_sim   [m, k] dense, of `dtype`; d_idx [m, k] dense int64 = index_offset + column of S.
 * Arithmetic -- the contract; tests rebuild it bit for bit.  For target j and source i, every operation rounded once
 * in T, no contraction (the library is built with -ffp-contract=off), the division IEEE:
 *     dot = 0;  for u = 0 .. users - 1 (ascending):  dot = dot + t[u][j] * s[u][i]
 *     sim = dot / (tnorm[j] * snorm[i])            one product of norms, one division
 *     sim = NaN -> +0,  +inf -> the largest finite T,  -inf -> the most negative finite T         (np.nan_to_num)
 * which is the reference's local_ratings.T.dot(remote_ratings) / local_item_norm.dot(remote_item_norm) and its
 * nan_to_num.  An item of norm 0 therefore has similarity 0 with every item, itself included.  The bits of a
 * similarity depend on the two columns and the two norms alone: not on the grid, `splits`, index_offset, or the place
 * of either item in a block.
 * Selection: per target the k best by the total order (similarity descending, index ascending); equal similarities go
 * to the lower index.  A target is NOT excluded from its own list (the reference keeps it).  If fewer than k sources
 * exist (ns < k) the trailing slots hold -inf and index -1; after nan_to_num no similarity is -inf, so the padding
 * cannot be mistaken.  The output is bit-identical for every value of `splits` and for every banding of the targets:
 * a band of targets computed alone gives the bits the whole gives.  No atomics of any kind; a repeated call gives the
 * same bits.
 *   splits  0: the library chooses from (m, ns, k) alone -- r = min(ceil(512 / ceil(m / 64)), ceil(ns / max(4 k, 64)),
 *           64), then the fewest ranges that need as many passes of 64 sources as r does: with p = ceil(ceil(ns / r)
 *           / 64), ranges = ceil(ns / (64 p)) (800 x 800, k = 10: 13 ranges of 61 or 62 sources; 8192 x 8192: 4;
 *           ns <= 64: 1); s >= 1: the sources are cut into exactly min(s, ns) ranges of
 *           columns, range g = columns floor(g ns / ranges) .. floor((g + 1) ns / ranges) - 1, each searched by its own
 *           workgroups, whose candidate lists go to the workspace and are merged by the code of sp_item_topk_merge.
 * Kernel (vector pipe only).  A workgroup of 256 threads owns 64 targets and streams its range of sources through LDS
 * 64 at a time in chunks of 16 users: a chunk of either operand is sixteen contiguous 64-item runs of the table, one
 * per wave and step, stored user-major with a row pitch of 68 -- no transpose; the next chunk's loads are in flight in
 * registers while this one is used.  Every thread holds a 4 x 4 block of partial inner products, one accumulator per
 * pair.  After the last user the thread finishes its 16 similarities; each is compared with its target's k-th best
 * and only survivors are inserted into the target's sorted list in LDS, by the wave that owns the target, together.
 * No workgroup waits for another.  Dynamic LDS: 2 * 16 * 68 elements + 64 k (element + 4) bytes (113 KiB in fp64 at
 * k = 128).  d_ws: sp_item_topk_workspace_bytes(...) bytes for the same arguments: 0 with one range or m = 0 (d_ws may
 * then be NULL), else ranges * m * k similarities (rounded up to 256 bytes) and as many int64. */
size_t sp_item_topk_workspace_bytes(int32_t dtype, int64_t users, int64_t m, int64_t ns, int32_t k, int32_t splits);
int sp_item_topk(int32_t dtype, const void* d_T, int64_t ldt, const void* d_tnorm, int64_t m, const void* d_S, int64_t lds,
                 const void* d_snorm, int64_t ns, int64_t users, int32_t k, int64_t index_offset, int32_t splits,
                 void* d_sim, int64_t* d_idx, void* d_ws, size_t ws_bytes, void* stream);

/* sp_item_topk_merge: every row has `cands` candidates (sim, idx) in any order, row-major with ldc >= cands elements
 * between rows in both arrays; entries with idx < 0 are padding and are ignored, and so are entries whose similarity is
 * NaN.  Writes the k best by (similarity descending, idx ascending) to d_sim / d_idx ([m, k] dense), padded with
 * -inf / -1 as above.  The inputs are not written and must not overlap the outputs.  Used for the split path inside
 * sp_item_topk, for the source steps of a column band and for the candidates of several tiles or ranks.  One wave
 * per row.  m = 0 and cands = 0 are accepted. */
int sp_item_topk_merge(int32_t dtype, const void* d_cand_sim, const int64_t* d_cand_idx, int64_t ldc, int64_t m,
                       int64_t cands, int32_t k, void* d_sim, int64_t* d_idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_CF_H_ */
