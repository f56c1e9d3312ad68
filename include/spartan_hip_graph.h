/* C-ABI of the graph kernels in libspartan_hip_extras.so (csrc/apsp.hip; `make extras`).  A header of its own, bound
 * as _hip.EXPORTS_GRAPH: the sets of functions the other extras headers declare are fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_GRAPH_H_
#define SPARTAN_HIP_GRAPH_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sp_apsp: all-pairs shortest paths, in place on the row-major n x n matrix D (ldd >= n elements between rows) -- the
 * geodesic step of the reference's Isomap (spartan/examples/sklearn/manifold/isomap.py, there a Dijkstra per source
 * row in sklearn/util/graph_shortest_path.pyx) as a blocked Floyd-Warshall.
 *   dtype   SP_F32 | SP_F64 (anything else is refused: convert with astype first).
 *   entry   D[i][j] = length of the edge i -> j, >= 0, +inf for "no edge" (a directed graph; a symmetric D is the
 *           undirected one).  The diagonal is ignored and taken as 0.
 *   return  D[i][j] = length of the shortest path i -> j, +inf where there is none, 0 on the diagonal.  Nothing outside
 *           the n x n box is written.  n = 0 and n = 1 are accepted.
 * Arithmetic: a candidate is t = D[i][k] + D[k][j], ONE rounded add in the matrix's precision, and it replaces
 * D[i][j] only if t < D[i][j]: every stored value is the rounded sum of a real path, and inf + x never wins.  A
 * symmetric input gives a bit-symmetric output.
 *   d_info  a device int32 the call writes: 0, or 1 if an off-diagonal entry is NaN or negative (one n^2 launch
 *           before the rounds, which also zeroes the diagonal; the word itself is cleared by a memset node ahead of
 *           it).  The rounds run regardless -- the launch sequence is fixed on the host, nothing waits for the device
 *           -- and D is unspecified when info is 1.
 * Blocks of 64; round kb = 0 .. ceil(n / 64) - 1 is three launches: the diagonal block closes on itself in LDS (one
 * workgroup); the 2 (nb - 1) blocks of block row and block column kb, each with its sequential k loop in LDS; every
 * other block takes min(C, A (x) B) in the (min, +) semiring, A = D[i, kb], B = D[kb, j] staged through LDS, a 4 x 4
 * patch of C per thread, no barrier inside the k loop.  A ragged last block is padded with +inf in LDS and its stores
 * are guarded.  1 + 3 ceil(n / 64) launches (fewer for one block); no workgroup waits for another. */
int sp_apsp(int32_t dtype, void* d_D, int64_t ldd, int64_t n, int32_t* d_info, void* stream);

/* sp_graph_from_knn: the dense undirected graph sp_apsp takes, from the (dist, idx) pair of a neighbour search: both
 * [n, k] with ldk >= k elements between rows, dist of `dtype` (SP_F32 | SP_F64) and >= 0, idx int64.  W [n, n] (ldw >= n)
 * is filled with +inf and 0 on the diagonal; then for every listed pair W[i][j] = W[j][i] = the smallest weight stated
 * for it in either direction (for non-negative floats the bit pattern orders as the value: an unsigned integer atomic
 * min).  Entries with idx < 0 are padding; idx >= n is a caller error the kernel skips, and so is idx = the row itself.
 * Two launches: fill, scatter.  n = 0 and k = 0 are accepted. */
int sp_graph_from_knn(int32_t dtype, const void* d_dist, const int64_t* d_idx, int64_t ldk, int64_t n, int64_t k,
                      void* d_W, int64_t ldw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_GRAPH_H_ */
