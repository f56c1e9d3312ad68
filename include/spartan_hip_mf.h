/* C-ABI of the stochastic-gradient matrix factorisation's tile body in libspartan_hip_extras.so (csrc/sgd_mf.hip;
 * `make extras`).  A header of its own, bound as _hip.EXPORTS_MF: the sets of functions the other headers declare are
 * fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_MF_H_
#define SPARTAN_HIP_MF_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest rank f (the reference's comment: 1 .. 500); any larger f is refused */
#define SP_MF_MAX_F 512
/* a level of the schedule with at least this many ratings is WIDE and gets a launch of its own; narrower levels are
 * NARROW and consecutive ones share one workgroup in one launch (profiles/netflix_notes.md: where the two costs cross) */
#define SP_MF_WIDE 64

/* The sequence.  The tile body of the reference's Netflix SGD (spartan/examples/netflix_core.pyx, _sgd_inner) on a tile
 * of ratings [m, n] in canonical CSR -- int64 indptr [m + 1], int32 indices ascending inside a row without duplicates,
 * values of type T = float or double -- with the factors U [m, f] and M [n, f] of type T, row-major with leading
 * dimensions ldu, ldm >= f, updated IN PLACE.  For each stored entry (i, j, r) in the tile's stored order (rows
 * ascending, columns ascending inside a row), every operation rounded once in T, no contraction:
 *     g    = dot(U_i, M_j)          d = r - g
 *     U_ik = U_ik + (U_ik * d) * lr      for every k
 *     M_jk = M_jk + (M_jk * d) * lr      for every k        lr = T(learning rate)
 * (each factor row is scaled by itself: what the reference's compiled loop does).  A stored entry whose value is 0 is a
 * rating like any other.
 * dot(p, q) has an order that depends on f alone: L lanes, L = 8 for f <= 16, 16 for f <= 64, 64 above.  Lane l
 * starts at +0 and adds p_k * q_k (a multiply, then an add) for k = l, l + L, ... in ascending order (a lane without a
 * k keeps +0); the L lane sums are added as a balanced tree, partners at distance L / 2 first, then L / 4, ..., 1.
 * abs_err, where given, is [nnz] in the tile's entry order: abs_err[e] = |d| of entry e as the sequence sees it.
 * The contract: the result is bit-identical to executing the sequence one entry at a time.  It does not depend on the
 * schedule, on SP_MF_WIDE, on the grid or on the number of workgroups; a call repeated on the same operands gives the
 * same bits; there are no atomics.  (Two entries that share neither their row nor their column touch disjoint memory,
 * so the schedule below only ever runs such entries at once.)
 * Special values follow the arithmetic: a NaN or infinite rating makes both of its rows NaN (or what IEEE gives),
 * later entries that touch those rows pass it on, entries that touch neither are unaffected.
 *
 * The schedule (host code: no device is needed).  level(e) = 1 + max(level of the previous entry of e's row, level of
 * the previous entry of e's column), 1 where there is neither; the entries of one level are independent.  The plan
 * is ONE block of bytes, the same on the host and (copied as it is) on the device:
 *     int64 head[16]    SP_MF_PLAN_MAGIC, m, n, nnz, levels, segments, used bytes, then the BYTE offsets of the five
 *                       arrays below (entry, row, col, level_off, segment), then SP_MF_WIDE as it was built with; 0s
 *     int32 entry[nnz]  the entries in level order (inside a level: ascending entry index), as entry index
 *     int32 row[nnz]    and their rows
 *     int32 col[nnz]    and columns
 *     int32 level_off[levels + 1]   level v (0-based) owns the positions level_off[v] .. level_off[v + 1] - 1
 *     int32 segment[segments][4]    (kind, first level, last level + 1, 0): kind SP_MF_SEG_WIDE is ONE level of at
 *                       least SP_MF_WIDE entries; kind SP_MF_SEG_NARROW is a maximal run of consecutive narrower
 *                       levels.  The segments tile 0 .. levels in order.
 * sp_sgd_mf_plan_bytes: an upper bound of the plan's size for a tile (0 for sizes that are refused); the bytes in use
 * are head[6].  sp_sgd_mf_plan refuses (non-zero, nothing promised about h_plan): negative sizes, m or n >= 2^31,
 * nnz >= 2^31, `bytes` below sp_sgd_mf_plan_bytes, indptr[0] != 0, indptr[m] != nnz, an indptr that is not monotone,
 * an index outside 0 .. n - 1 (and NULL pointers where they are read).  It does not check that a row's indices ascend:
 * a tile whose rows repeat a column still gets a valid schedule of ITS stored order. */
#define SP_MF_PLAN_MAGIC 0x314e4c50464d5053LL /* "SPMFPLN1" */
#define SP_MF_SEG_NARROW 0
#define SP_MF_SEG_WIDE 1
size_t sp_sgd_mf_plan_bytes(int64_t m, int64_t n, int64_t nnz);
int sp_sgd_mf_plan(int64_t m, int64_t n, int64_t nnz, const int64_t* h_indptr, const int32_t* h_indices, void* h_plan,
                   size_t bytes);

/* sp_sgd_mf_host: the sequence as a plain single-threaded loop on HOST arrays -- the same arithmetic, dot order
 * included -- in the order h_order [nnz] (entry indices; each entry once) or in tile order when it is NULL.  The fast
 * oracle of large cases and the CPU yardstick of tools/bench_netflix.py; in a plan's entry order it gives the bytes of
 * tile order.  Refusals: those of sp_sgd_mf below (on the host pointers), an indptr that is not monotone from 0 to nnz,
 * an index outside 0 .. n - 1, an h_order entry outside 0 .. nnz - 1. */
int sp_sgd_mf_host(int32_t dtype, int64_t m, int64_t n, int64_t f, int64_t nnz, const int64_t* h_indptr,
                   const int32_t* h_indices, const void* h_vals, void* h_U, int64_t ldu, void* h_M, int64_t ldm, double lr,
                   void* h_abs_err, const int32_t* h_order);

/* sp_sgd_mf: the sequence on the device, one call per tile.  d_vals [nnz] are the tile's values (type T); h_plan is
 * the plan of the tile's structure and d_plan a copy of its first head[6] bytes in device memory (4-byte aligned
 * offsets inside it: allocate it 8-byte aligned); d_U, d_M as above, d_abs_err NULL or [nnz].  It walks the segment
 * table and launches each segment on `stream` with plain launches, in order: nothing else synchronises, no workgroup
 * ever waits for another, no flags, no cooperative launch.  *launched (where not NULL) <- the number of launches.
 * Refused, with nothing launched: a dtype other than SP_F32 / SP_F64, f outside 1 .. SP_MF_MAX_F, ldu < f or ldm < f,
 * negative sizes, an lr that is not finite (as given or as T), a plan whose head does not carry the magic number or
 * the sizes m, n, nnz (or whose offsets leave its bytes), and with nnz > 0 NULL d_vals, d_plan, d_U or d_M.  nnz = 0
 * launches nothing.
 * Kernels (vector pipe only; L lanes to a rating, so a wave handles 64 / L ratings at once; lane l of a rating gathers
 * the value through the entry index, reads the elements l, l + L, ... of both rows, forms dot as stated, and writes the
 * same elements of both rows back):
 *   mf_wide_kernel    one level: workgroups of 256 threads, 256 / L ratings each, no barrier; the kernel boundary
 *                     orders it against the segments before and after.
 *   mf_narrow_kernel  a run of narrow levels: ONE workgroup of 256 threads loops over the run's levels with a
 *                     workgroup barrier between them.  Rows written by one wave and read by another wave of the same
 *                     workgroup stay on one compute unit, whose vector L1 all its waves share. */
int sp_sgd_mf(int32_t dtype, int64_t m, int64_t n, int64_t f, int64_t nnz, const void* d_vals, const void* d_plan,
              const void* h_plan, void* d_U, int64_t ldu, void* d_M, int64_t ldm, double lr, void* d_abs_err,
              int64_t* launched, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_MF_H_ */
