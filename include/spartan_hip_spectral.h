/* C-ABI of the affinity / normalised-Laplacian kernels of spectral clustering in libspartan_hip_extras.so
 * (csrc/spectral.hip; `make extras`).  A header of its own, bound as _hip.EXPORTS_SPECTRAL: the sets of functions the
 * other headers declare are fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_SPECTRAL_H_
#define SPARTAN_HIP_SPECTRAL_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the measures (`metric`) */
#define SP_AFF_RBF 0
#define SP_AFF_EUCLIDEAN 1
#define SP_AFF_MANHATTAN 2

/* rows and columns of a tile, and the fewest blocks of 64 columns a column range of sp_affinity_degree holds */
#define SP_AFF_TILE 64
#define SP_AFF_RANGE_BLOCKS 4
#define SP_AFF_MAX_RANGES 64

/* The hot loop of the reference's spectral clustering (spartan/examples/spectral_clustering.py:61-103:
 * _row_similarity_mapper, sum(A, axis=1), _laplacian_mapper) without the affinity matrix A ever being stored:
 *     a_ij = measure(x_i, y_j)         D_i = sum_j a_ij         s_i = 1 / sqrt(D_i), 1 where D_i is 0  (on the host)
 *     L_ij = a_ij * (s_i * s_j),  L_ii = 1
 * sp_affinity_degree finds D while the affinities stay in registers; sp_affinity_matrix recomputes them and writes L
 * (or, without S, the plain A) exactly once.
 *   dtype   SP_F32 | SP_F64 for every operand alike (anything else is refused: convert with astype first).  All
 *           arithmetic is done in it, call it T.
 *   metric  SP_AFF_RBF        a = exp(-(g * d2)),  g = T(gamma) rounded once (the reference always runs gamma = 1)
 *           SP_AFF_EUCLIDEAN  a = sqrt(d2)
 *           SP_AFF_MANHATTAN  a = d1
 *           with d2_ij = sum_f (x_if - y_jf)^2 in the DIFFERENCE form of sp_knn and sp_fuzzy_step and d1_ij =
 *           sum_f |x_if - y_jf|: one subtract, one multiply (or one absolute value) and one add per feature, no
 *           contraction, the features added in ascending order f = 0 .. d - 1 onto ONE accumulator that starts at 0 --
 *           the same for every pair wherever it falls in a tile or a band.  (x - y)^2 and |x - y| do not change when
 *           the operands are exchanged, so a_ij and a_ji have the same bits when X and Y are the same points.  exp /
 *           expf and sqrt are the functions of the map kernel's EXP and SQRT opcodes; sqrt is IEEE.  Anything else
 *           is refused ('scaled_euclidean' of the reference has no definite value, see examples/spectral_clustering.py).
 *   gamma   finite in T (|gamma| at most the largest finite T), else refused; used by SP_AFF_RBF only.
 *   X [m, d], Y [n, d]   row-major, ldx, ldy >= d elements between rows; neither is written.  m = 0 and d = 0 are
 *           accepted (with d = 0 every distance is 0); n = 0 gives D = 0 and an empty matrix.  A refusal launches nothing.
 *
 * sp_affinity_degree: D_i = sum_j a(x_i, y_j) over ALL n rows of Y, D [m] contiguous.  Nothing of size m x n is stored.
 * Order of a row's sum, three levels:
 *   - the columns are taken in blocks of 64, j = 64 b .. 64 b + 63 (a column at or beyond n adds +0).  In a block the 16
 *     groups of four consecutive columns are each summed in ascending order onto 0;
 *   - the 16 group sums g_0 .. g_15 are added as a balanced tree, (g_t + g_{t^1}) first, then pairs of those at
 *     distance 2, 4 and 8 (the tree of z_i in spartan_hip_fuzzy.h);
 *   - the blocks' sums are added in ascending order onto an accumulator that starts at 0.
 * Column ranges: the nb = ceil(n / 64) blocks are cut into `ranges` = min(max(floor(nb / 4), 1), 64) ranges -- a number
 * chosen from n alone, NEVER from m -- range g = blocks floor(g nb / ranges) .. floor((g + 1) nb / ranges) - 1, each
 * worked on by workgroups of its own.  With more than one range the ranges' sums go to the workspace and
 * sp_partial_sum adds them in ascending range order onto range 0's.  The bits of D_i therefore depend on row i of X
 * and on Y alone: not on the row's neighbours, its place in X, or m -- a band of rows computed alone gives the bits
 * the whole gives.  No atomics; a call repeated on the same operands gives the same bits.
 *   d_ws    sp_affinity_degree_workspace_bytes(...) bytes for the same arguments: ranges * m elements with more than
 *           one range, 0 (and d_ws may be NULL) with one.  A workspace that is too small is refused.
 *
 * sp_affinity_matrix: out [m, n] with ldo >= n elements between rows; row i of X is point r0 + i of the n points Y
 * (r0 < 0 or r0 + m > n is refused).
 *   with S [n]     out_ij = a_ij * (s_{r0+i} * s_j): the product of the two scales first, then ONE multiply; then
 *                  out_{i, r0+i} = 1 exactly (the reference sets L's diagonal to 1 after normalising; with 'rbf' the
 *                  leading eigenvalues are therefore about 1.93, not 1).  This association differs from the reference's
 *                  (s_i a_ij) s_j by a rounding; it is chosen so that L is SYMMETRIC BIT FOR BIT (s_i * s_j commutes,
 *                  a_ij == a_ji): the Lanczos driver is told that the matrix is symmetric.
 *   S == NULL      the plain a_ij, nothing overwritten.
 * An element's bits depend on its two points, its two scales and whether it is on the diagonal, nothing else.
 *
 * Kernels (vector pipe only; no atomics; no workgroup waits for another):
 *   affinity_degree_kernel   a workgroup of 256 threads owns 64 rows of X and a column range; it sweeps the range's
 *                            rows of Y 64 at a time through sp_d2_tile (LDS, chunks of 16 features, every thread a
 *                            4 x 4 block of distances), applies the measure in registers and sums over the 16 lanes of
 *                            a row by a butterfly: no LDS and no barrier beyond the tile's.
 *   sp_partial_sum_kernel    only with more than one range.
 *   affinity_matrix_kernel   one workgroup per 64 x 64 tile of `out`: the same distance tile over all d features, the
 *                            measure, the scale and the diagonal in registers; a thread's four consecutive columns
 *                            leave in aligned 16-byte stores (one in fp32, two in fp64) where `out` and ldo *
 *                            sizeof(T) are multiples of 16 bytes and all four columns exist, one by one otherwise.
 * 'manhattan' is a parameter of sp_d2_tile (sp_extras_common.hpp) whose default leaves the squared-distance
 * instantiations of sp_fuzzy_step unchanged. */
size_t sp_affinity_degree_workspace_bytes(int32_t dtype, int64_t m, int64_t n, int64_t d);
int sp_affinity_degree(int32_t dtype, int32_t metric, double gamma, const void* d_X, int64_t ldx, int64_t m,
                       const void* d_Y, int64_t ldy, int64_t n, int64_t d, void* d_D, void* d_ws, size_t ws_bytes,
                       void* stream);
int sp_affinity_matrix(int32_t dtype, int32_t metric, double gamma, const void* d_X, int64_t ldx, int64_t m, int64_t r0,
                       const void* d_Y, int64_t ldy, int64_t n, int64_t d, const void* d_S, void* d_out, int64_t ldo,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_SPECTRAL_H_ */
