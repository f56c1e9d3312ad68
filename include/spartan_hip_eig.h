/* C-ABI of the symmetric eigensolver in libspartan_hip_extras.so (csrc/linalg.hip, beside sp_potrf / sp_trsm_rlt of
 * spartan_hip_extras.h; `make extras`).  A header of its own, bound as _hip.EXPORTS_EIG: the set of functions
 * spartan_hip_extras.h declares is fixed, name by name, by tests/test_linalg_gpu.py. */
#ifndef SPARTAN_HIP_EIG_H_
#define SPARTAN_HIP_EIG_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sp_syevj: eigenvalues and eigenvectors of a symmetric n x n tile, A . V = V . diag(W) -- the np.linalg.eig of the
 * reference's stochastic SVD (spartan/examples/ssvd/ssvd.py:38, on the small K x K matrix B . B^T) and with it of its
 * PCA (examples/pca.py).  dtype: SP_F32 | SP_F64 (anything else is refused: convert with astype first).  d_A is
 * row-major with lda >= n; only its lower triangle is read (it is mirrored into the workspace) and d_A is NOT written.
 * d_W receives the n eigenvalues in ascending order (LAPACK's), d_V (row-major, ldv >= n) the eigenvectors as columns
 * in the same order.  The matrix may be indefinite.  Method: cyclic two-sided Jacobi, the pairs of a sweep taken in
 * the n - 1 (n even) or n (n odd, one index sits out) rounds of a round-robin tournament, the rotations of a round
 * disjoint and applied together; rotation by Rutishauser's formulas with IEEE-rounded square root and divide.  Orders
 * up to 64 (fp32) / 63 (fp64) run whole sweeps in the LDS of one workgroup; above that one launch per round works out
 * of place between two buffers of the workspace and no workgroup waits for another.  After every sweep the host reads
 * one 8-byte word (converged or not, sweeps done) and stops when off(A)_F <= n u ||A||_F, u = 2^-24 | 2^-53; after 64
 * sweeps without that it stops with *d_info = 1 (a device int32, otherwise 0; a NaN in A ends there), W and V then
 * hold the last iterate.  *sweeps_out (HOST memory, may be NULL) receives the number of sweeps.  The call waits for
 * the stream once per sweep (once per 8 sweeps in LDS).  n = 0 is accepted; n = 1 returns W = A, V = 1. */
size_t sp_syevj_workspace_bytes(int32_t dtype, int64_t n);
int sp_syevj(int32_t dtype, void* d_A, int64_t lda, int64_t n, void* d_W, void* d_V, int64_t ldv, void* d_ws,
             size_t ws_bytes, int32_t* d_info, int32_t* sweeps_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_EIG_H_ */
