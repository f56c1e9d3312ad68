/* C-ABI of the alternating-least-squares tile kernel in libspartan_hip_extras.so (csrc/als.hip; `make extras`).  A
 * header of its own, bound as _hip.EXPORTS_ALS: the sets of functions the other headers declare are fixed, name by
 * name, by tests. */
#ifndef SPARTAN_HIP_ALS_H_
#define SPARTAN_HIP_ALS_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the largest number of features sp_als_solve takes (a larger one is refused) */
#define SP_ALS_MAX_F 64

/* sp_als_solve: one half-step of alternating least squares -- for every row i of the ratings R [m, n] the solution
 * x_i of the f x f normal equations A_i x_i = b_i built from the factors Y [n, f]; the tile body of the reference's
 * spartan/examples/als.py (_solve_U_or_M_mapper: a Python loop over rows around scipy.linalg.lstsq) as one fused
 * pass that reads R once and writes only X [m, f].
 *   dtype   SP_F32 | SP_F64 (anything else is refused: convert with astype first).  All arithmetic is done in it; la
 *           and alpha are rounded to it once.
 *   R, Y    row-major, ldr >= n and ldy >= f elements between rows; neither is written.  X: ldx >= f.
 *   f       1 <= f <= SP_ALS_MAX_F.  m = 0 is accepted; n = 0 gives X = 0 in both modes.  m <= 2^31 - 2.
 * Explicit mode (implicit == 0; the reference's _als_solver), with S_i = { j : r_ij != 0 }:
 *   A_i = sum_{S_i} y_j y_j^T + (la * |S_i|) I        b_i = sum_{S_i} r_ij y_j        x_i = 0 exactly if S_i is empty
 * Implicit mode (the reference's _implicit_feedback_als_solver):
 *   A_i = (sum_j (alpha r_ij) y_j y_j^T + Y^T Y) + la I        b_i = sum_{r_ij > 0} (1 + alpha r_ij) y_j
 *   Y^T Y is formed once per call by a pre-pass into the workspace: plain FMAs over fixed ranges of items (their length
 *   a function of n alone), the ranges' partial sums added in ascending order; no atomics.
 * An item whose rating is 0 contributes nothing in either mode.  Every sum is a chain of FMAs onto accumulators that
 * start at 0; the order in which the items of a row are added is fixed by n and f alone, so row i of X depends only
 * on row i of R, on Y and on the scalars, and its bits do not change with the other rows of the call, with the row's
 * place in a workgroup, or with ldr, ldy, ldx.
 * Solve: Cholesky of A_i (lower, left-looking, IEEE sqrt and divide), forward and back substitution.  If a pivot is
 * not > 0 (the comparison fails for NaN as well, so a NaN rating fails its row) or b_i is not finite, the row of X is
 * filled with NaN and *d_info is set.
 *   d_info  a device int32 the CALLER zeroes: if it is 0 when the call's last kernel runs it receives 1 + the lowest
 *           failing row of this call; a nonzero value is left alone, and 0 is never written.
 *   d_ws    sp_als_solve_workspace_bytes(...) bytes for the same arguments (never 0). */
size_t sp_als_solve_workspace_bytes(int32_t dtype, int64_t m, int64_t n, int32_t f, int32_t implicit);
int sp_als_solve(int32_t dtype, const void* d_R, int64_t ldr, int64_t m, int64_t n, const void* d_Y, int64_t ldy,
                 int32_t f, double la, double alpha, int32_t implicit, void* d_X, int64_t ldx, int32_t* d_info,
                 void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_ALS_H_ */
