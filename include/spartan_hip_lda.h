/* C-ABI of the LDA (CVB0) step kernel in libspartan_hip_extras.so (csrc/lda.hip; `make extras`).  A header of its own,
 * bound as _hip.EXPORTS_LDA: the sets of functions the other headers declare are fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_LDA_H_
#define SPARTAN_HIP_LDA_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* documents a workgroup of the gamma kernel owns (the unit in which `splits` cuts the documents), terms a workgroup of
 * the delta kernel owns, and the largest number of topics */
#define SP_LDA_DOCS 64
#define SP_LDA_TERMS 64
#define SP_LDA_MAX_K 128

/* sp_lda_step: the tile body of the reference's LDA (spartan/examples/lda.py:7-52, 72-80, 100-110; Mahout's collapsed
 * variational Bayes, CVB0) on one tile X [V, D] of terms x documents against the whole topic / term counts N [k, V]:
 *     ts_t = sum_j |N_tj|                                  den_t = ts_t + eta V
 *     per document d:   gamma_t = 1 / k
 *       repeat `iters` times:
 *         for every term j with x_jd != 0:
 *           p_tj = (N_tj + eta) (gamma_t + alpha) / den_t ;    q_tj = x_jd p_tj / sum_t p_tj
 *         c_t = sum_j |q_tj| ;    gamma_t = c_t / sum_t |c_t|
 *       doc_topics[d, :] = gamma           delta[:, j] += q[:, j] of the LAST iteration
 * (the q of the last iteration comes from the gamma that ENTERED it).  The reference's train mapper yields N + delta,
 * its inference mapper doc_topics.
 * Form.  The per-document loops are two small matrix products around an elementwise quotient.  With
 *     A[t, j] = (N_tj + eta) / den_t        B[d, t] = gamma_dt + alpha        S[j, d] = sum_t A[t, j] B[d, t]
 *     W[j, d] = x_jd / S[j, d] where x_jd != 0, no pair otherwise
 *     c_dt = B[d, t] . sum_j |A[t, j]| |W[j, d]|         delta_tj = A[t, j] . sum_d W[j, d] B[d, t]
 * which is the reference's arithmetic in another association (p_tj / sum_t p_tj = A B / S), a few ulp away from it.
 * Nothing of size V x D is stored, let alone the reference's k x V model per document.
 *   dtype   SP_F32 | SP_F64 for X, N, delta and doc_topics alike (anything else is refused: convert with astype first).
 *           All arithmetic is done in it, call it T: T(alpha), T(eta), T(V) and 1 / k = T(1) / T(k) are each rounded
 *           once.
 *   X       [V, D] row-major, ldx >= D elements between rows; N [k, V], ldn >= V; neither is written.  X finite is a
 *           precondition of the caller.  A negative x counts with |x| in c and with its sign in delta, as in the
 *           reference.
 *   Refused, with nothing launched: k outside 1 .. 128, iters < 1, alpha or eta not finite or not > 0 (with either not
 *           > 0 the reference's "non-zero of topic 0's row" test stops meaning "non-zero term of the document"),
 *           leading dimensions below the row length, splits < 0.  D = 0 is accepted (delta = 0, doc_topics empty), and
 *           so is V = 0 (every document is empty).
 *   d_delta [k, V] with ldd >= V, or NULL: the sum over the tile's documents of the last iteration's q, from 0.
 *   d_doc_topics [D, k] with ldt >= k, or NULL.
 * Empty document.  A document with no non-zero term has c = 0, so its row of doc_topics is 0 / 0 = NaN, as in the
 * reference.  It adds exactly 0 to delta: its stored B is written as 0, so its (absent) pairs never meet the NaN.  A
 * term no document of the tile holds gets a delta column of zeros.
 * Orders of summation (no contraction anywhere, no atomics; a repeated call gives the same bits):
 *   ts_t    thread i of 256 adds j = i, i + 256, .. in ascending order onto 0; the 256 partial sums are added as a
 *           binary tree, i with i + 128, then + 64, .. + 1.
 *   S[j, d] t = 0 .. k - 1 in ascending order onto one accumulator that starts at 0 (topics up to the next of 16, 32,
 *           64, 128 add a . b = 0 . 0).
 *   c_dt    the terms j = 0 .. V - 1 in ascending order onto one accumulator that starts at 0, a term with x = 0
 *           adding |a| . 0; then one multiplication by B[d, t].
 *   sum_t c t = 0 .. k - 1 in ascending order onto 0.
 *   Row d of doc_topics therefore depends on column d of X and on N alone: not on the document's neighbours, its
 *   position, D or `splits`.
 *   delta   the documents are cut into `ranges` ranges of whole blocks of 64 documents, range g = blocks
 *           floor(g nb / ranges) .. floor((g + 1) nb / ranges) - 1 with nb = ceil(D / 64); inside a range the documents
 *           are added in ascending order onto accumulators that start at 0, then comes one multiplication by A[t, j];
 *           with more than one range the ranges' [k, V] partials go to the workspace and a combine kernel adds them in
 *           ascending range order onto range 0's.
 *   splits  0: the library chooses `ranges` from V, D and k only; s >= 1: exactly min(s, nb) ranges (1 when D = 0).
 *           Ranges are needed: at the reference's own test shape (V = 160) there are three blocks of 64 terms for 256
 *           compute units.
 * Kernels (vector pipe only; no workgroup waits for another).  KP is k rounded up to 16, 32, 64 or 128; a thread
 * holds KP / 16 topics.
 *   lda_prep_kernel     a workgroup per topic: ts, then A to the workspace as [V][KP], the topics of a term contiguous.
 *   lda_gamma_kernel    a workgroup of 256 threads owns 64 documents, B [KP][64] in LDS.  Per inner iteration it sweeps
 *                       the terms in chunks of TC: the X chunk (rows of X are contiguous over documents: the loads
 *                       coalesce) and the A chunk into LDS, the TC x 64 tile of S in registers (TC / 16 x 4 per thread),
 *                       the quotient in place of x, then c [64, KP] in registers, a thread 4 documents x KP / 16 topics
 *                       (32 accumulators at k = 128); then it normalises.  It writes the B that entered the last
 *                       iteration to the workspace (only when delta is wanted) and gamma to d_doc_topics.
 *                       The next chunk is in flight in registers while one is worked on.
 *                       LDS, in elements with rows padded by 4: B KP x 68, A chunk KP x (TC + 4), X / W chunk TC x 68,
 *                       64 sums, 64 flags of 4 bytes.  TC is 64 up to KP = 64 (fp32: 52.7 KB).  At KP = 128, fp32 with
 *                       TC = 64 would be 87.6 KB, one workgroup per compute unit of 160 KB; TC = 32 is 62.5 KB, two.
 *                       fp64 with TC = 64 would be 174.8 KB at KP = 128, more than a compute unit has, so fp64 takes
 *                       TC = 32 throughout: 124.7 KB at KP = 128.
 *   lda_delta_kernel    a workgroup per (64 terms) x (document range), its A block [KP][64] in LDS.  Per sub-block of
 *                       DC documents (DC = TC: the same budget, 62.5 KB and 124.9 KB at KP = 128) it loads the stored
 *                       B and X, the next sub-block in flight in registers, recomputes the S tile, forms the signed
 *                       quotient, and accumulates acc [64 terms, KP] in registers, a thread 4 terms x KP / 16 topics; it
 *                       multiplies by A at the end.
 *   sp_partial_sum_kernel  only with more than one range (and to write the zeros of D = 0).
 * Cost: S is computed iters + 1 times (iters without delta), 2 V D KP flops each, beside the 2 V D KP of each
 * accumulation: the price of storing nothing of size V x D.
 *   d_ws    sp_lda_step_workspace_bytes(...) bytes for the same arguments (never 0 for arguments that are taken): A,
 *           the stored B [D][KP], the ranges' partials. */
size_t sp_lda_step_workspace_bytes(int32_t dtype, int64_t V, int64_t D, int64_t k, int32_t iters, int32_t splits);
int sp_lda_step(int32_t dtype, const void* d_X, int64_t ldx, int64_t V, int64_t D, const void* d_N, int64_t ldn,
                int64_t k, double alpha, double eta, int32_t iters, int32_t splits, void* d_delta, int64_t ldd,
                void* d_doc_topics, int64_t ldt, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_LDA_H_ */
