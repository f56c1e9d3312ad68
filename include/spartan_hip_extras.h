/* C-ABI of libspartan_hip_extras.so: kernels behind operators that are NOT on the tile path this repository is
 * about (SURVEY.md section 2 marks them out of scope) but that the host framework still offers: sort, and the
 * dense factorisation kernels of the Cholesky and Cholesky-QR drivers.  Built by
 * `make extras` in spartan_amd/csrc (and by __graft_entry__.build()), not by the default `make`; the library links
 * against libspartan_hip.so (error reporting: sp_last_error()). */
#ifndef SPARTAN_HIP_EXTRAS_H_
#define SPARTAN_HIP_EXTRAS_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sp_sort_rows: np.sort / np.argsort along the LAST axis of a contiguous [rows, cols] tile -- the tile bodies of the
 * sort operators (spartan/expr/operator/sort.py:68-69 _sort_mapper, :137-138 _argsort_mapper, :24 / :65 the
 * flat np.sort of the sample sort; rows == 1 sorts a flattened tile).  Stable (np.argsort(kind='stable')), NaN
 * last, -0.0 == +0.0; d_out_vals (sorted values, may be NULL) and d_out_idx (int64 column of each sorted value,
 * may be NULL) are out of place.  dtype: SP_F32 | SP_F64 | SP_I32 | SP_I64.  Rows of <= 4096 32-bit elements are
 * sorted in LDS in one pass over HBM; anything else by an LSD radix sort of the whole tile (key bytes, then the
 * row of each position). */
size_t sp_sort_rows_workspace_bytes(int32_t dtype, int64_t rows, int64_t cols);
int sp_sort_rows(const void* d_in, int32_t dtype, int64_t rows, int64_t cols, void* d_out_vals, int64_t* d_out_idx,
                 void* d_ws, size_t ws_bytes, void* stream);

/* sp_potrf: Cholesky factorisation A = L . L^T of a symmetric positive definite n x n tile, in place -- the tile body
 * of the reference's blocked Cholesky (spartan/examples/cholesky.py:9-13, linalg.lapack.dpotrf(tile, lower=1)) and
 * the np.linalg.cholesky of its Cholesky-QR (examples/ssvd/qr.py:37).  dtype: SP_F32 | SP_F64 (anything else is
 * refused: convert with astype first).  d_A is row-major with lda >= n elements between rows; only its lower
 * triangle is read; on return the lower triangle holds L and the strict upper triangle is ZERO (scipy's clean=1).
 * *d_info (a device int32, written by the call) is 0, or the 1-based order of the first leading minor that is not
 * positive definite, as LAPACK's info: the kernels behind the failing pivot do nothing and the contents of A are
 * then unspecified (finite where the input was).  Square root and divide are IEEE-rounded.  Blocked on two levels,
 * left-looking: a block column of 256 takes its update from everything to its left in one call of sp_gemm_ws
 * (scratch: d_ws of sp_potrf_workspace_bytes(dtype, n) bytes, sized so that the product stays on the fp32 / fp64
 * MFMA tiers), below that diagonal blocks of 64 are factored in LDS by one workgroup.  n = 0 is accepted. */
size_t sp_potrf_workspace_bytes(int32_t dtype, int64_t n);
int sp_potrf(int32_t dtype, void* d_A, int64_t lda, int64_t n, void* d_ws, size_t ws_bytes, int32_t* d_info,
             void* stream);

/* sp_trsm_rlt: B <- X with X . L^T = B (right side, lower, transposed, non-unit): L n x n row-major with ldl, its upper
 * triangle not read; B m x n row-major with ldb, in place.  The reference's dtrtrs(A_kk, tile.T, lower=1).T
 * (cholesky.py:16-20) and Q = Y . R^-1 with R = L^T (ssvd/qr.py:40-43, there an explicit inverse).  Forward
 * substitution by blocks of 64 columns, L's blocks through LDS; a workgroup owns 128 rows of B and synchronises
 * with no other.  dtype: SP_F32 | SP_F64.  n = 0 and m = 0 are accepted. */
int sp_trsm_rlt(int32_t dtype, const void* d_L, int64_t ldl, int64_t n, void* d_B, int64_t ldb, int64_t m,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_EXTRAS_H_ */
