/* C-ABI of the all-pairs gravity kernel in libspartan_hip_extras.so (csrc/nbody.hip; `make extras`).  A header of its
 * own, bound as _hip.EXPORTS_NBODY: the sets of functions the other headers declare are fixed, name by name, by tests. */
#ifndef SPARTAN_HIP_NBODY_H_
#define SPARTAN_HIP_NBODY_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* sources in a block (the unit in which `splits` cuts the sources; also the targets of a workgroup), the interleaved
 * classes the sources of a block are dealt into (one per wave), and the workgroups the automatic choice of ranges
 * aims at */
#define SP_NBODY_BLOCK 64
#define SP_NBODY_WAVES 4
#define SP_NBODY_WORKGROUPS 1024

/* sp_nbody_accel: the accelerations of bodies r0 .. r0 + m - 1 under the gravity of ALL n bodies -- the n x n
 * expressions of the reference's spartan/examples/nbody.py move() (dx, dy, dz, r, the mask, three forces and their sums
 * over axis 0) without anything of size n x n.  For target j and source i != j, every operation rounded once in T:
 *     dx = x_i - x_j   (dy, dz alike)          q = (dx*dx + dy*dy) + dz*dz        r = sqrt(q)
 *     r  = r < rmin ? T(rmin) : r              (a NaN r stays NaN; the reference's mask with rmin = 1)
 *     w  = (T(g) * mass_i) / ((r * r) * r)     a_x[j] += w * dx   (a_y, a_z alike)
 * The reference computes G*m*dx / r**3 per component: three divisions and a pow.  Here w is divided once and r^3 is two
 * multiplications, which differs from the reference by a rounding or two per term (the tests' bound covers both).  No
 * contraction (the library is built with -ffp-contract=off); sqrt and the division are IEEE.
 *   dtype   SP_F32 | SP_F64 for all seven arrays (anything else is refused: convert with astype first).
 *   d_x, d_y, d_z, d_mass   contiguous [n]; never written.   d_ax, d_ay, d_az   contiguous [m]; written whole.
 *   Refused, with nothing launched: negative n, m or splits, r0 < 0 or r0 + m > n ("are not among"), a g that is not
 *           finite in T, an rmin that is not finite and > 0 in T, NULL inputs with n > 0 or NULL targets with m > 0
 *           ("required"), more workgroups than a launch takes, a workspace that is NULL or too small when one is needed.
 * Special values.  Source i == j and the padding of the last block (sources n .. 64 ceil(n / 64) - 1) add +0 to all
 * three sums whatever the coordinates are, so n = 1 gives zeros.  Coincident bodies have dx = 0, r = rmin and a term of
 * exactly 0.  A NaN coordinate makes every a NaN; an infinite one gives NaN where inf - inf or 0 * inf arises.  m = 0
 * launches nothing.
 * Order -- the contract; tests rebuild it term by term.  nb = ceil(n / 64) source blocks are cut into `ranges` ranges,
 * range g = blocks floor(g nb / ranges) .. floor((g + 1) nb / ranges) - 1.
 *   1. within a thread: for a target and a range, class c (0 .. 3) is ONE accumulator per component that starts at +0
 *      and takes the terms of the range's sources i with i mod 4 == c in ascending i (the +0 of i == j and of the
 *      padding included).
 *   2. across the waves that share a target: wave c of the workgroup holds class c; the four partials are combined
 *      through LDS as (p0 + p1) + (p2 + p3).
 *   3. across ranges: with one range that is a[j].  With more, the ranges' [3, m] results go to the workspace and
 *      sp_partial_sum_kernel adds them in ascending range order onto range 0's.
 * No atomics of any kind; a call repeated on the same operands gives the same bits.  The bits of a[j] depend on body j,
 * the n sources and (n, splits) only -- not on r0, m, or where in a workgroup the target sits: a band of targets
 * computed alone gives the bits the whole gives.
 *   splits  0: ranges = min(nb, ceil(1024 / nb)), from n alone (n = 1000: 16 ranges x 16 target blocks = 256
 *           workgroups; n >= 65536: one range); k >= 1: exactly min(k, nb) ranges.
 * Kernel (vector pipe only).  nbody_accel_kernel: a workgroup of 4 waves per (64 targets) x (range); lane l of every
 * wave holds target r0 + 64 b + l in registers.  A block of 64 sources is staged in LDS as (x, y, z, T(g) * mass), the
 * next block's loads in flight while this one is used (two LDS buffers, one barrier per block); wave c reads sources
 * c, c + 4, ... of it, every lane the same address (a broadcast read).  Only the blocks that hold one of the
 * workgroup's own targets or the padding pay for the selection of +0.  With more than one range sp_partial_sum_kernel
 * follows: one launch of it when d_ay - d_ax == d_az - d_ay >= m elements (rows of one [3, m'] array, as
 * HipBackend.nbody_accel allocates them), else two.
 *   d_ws    sp_nbody_accel_workspace_bytes(...) bytes for the same arguments: 0 with one range or m = 0 (d_ws may then
 *           be NULL), ranges * 3 * m elements otherwise. */
size_t sp_nbody_accel_workspace_bytes(int32_t dtype, int64_t n, int64_t m, int32_t splits);
int sp_nbody_accel(int32_t dtype, double g, double rmin, const void* d_x, const void* d_y, const void* d_z,
                   const void* d_mass, int64_t n, int64_t r0, int64_t m, void* d_ax, void* d_ay, void* d_az,
                   int32_t splits, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARTAN_HIP_NBODY_H_ */
