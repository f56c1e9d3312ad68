// Split tier of sp_gemm_ws (fp32): the contraction on the bf16 matrix pipe, which on gfx950 runs at 16 x the rate of
// the fp32 one (v_mfma_f32_16x16x32_bf16: 32 k of a 16 x 16 block per 16 cycles; v_mfma_f32_32x32x2_f32: 2 k of a
// 32 x 32 block per 64).  Included by gemm.hip.
//
// THE CUT.  Every fp32 operand is cut into three bf16 numbers, v = hi + mid + lo with hi = bf16(v), mid = bf16(v - hi),
// lo = bf16((v - hi) - mid), all conversions round-to-nearest-even.  bf16 keeps 8 significant bits, so for v in
// [2^e, 2^(e+1)) the first remainder is a multiple of ulp(v) = 2^(e-23) no larger than 2^(e-8) <= 2^-8 |v| -- 16 bits and
// a sign --, the second one no larger than 2^(e-16) <= 2^-16 |v| -- 8 bits and a sign: both subtractions are exact in fp32,
// lo is exact and the cut loses nothing, 24 significand bits as 8 + 8 + 8 (tests/test_gemm_split_cut.py shows it on the
// bit patterns).
//
// THE PRODUCTS.  a b = sum of the nine piece products; six are taken per 16 k, into one fp32 accumulator:
//     ah bh, ah bm, am bh, am bm, ah bl, al bh
// each EXACT in fp32 (8 x 8 significant bits).  The three left out are
//     |am bl| + |al bm| + |al bl| <= (2^-8 2^-16 + 2^-16 2^-8 + 2^-32) |a b| <= 2.004 u |a b|,   u = 2^-24:
// the size of the rounding of ONE fp32 product, and of either sign (summed over uniform data they cancel to
// 0.004 u sum|a b|).  They vanish altogether when a b is itself exact in fp32 (a with p significant bits and b with q,
// p + q <= 24: am bl != 0 needs p > 8 and q > 16, al bm != 0 p > 16 and q > 8), so integer-valued GEMMs whose fp32
// result is exact stay bit-exact here.
//
// THE BOUND.  With S = sum_k |a_k b_k|, the result differs from the exact product by
//   * the terms left out:                                        <= 2.004 u S
//   * the accumulation of the 6 K exact products in fp32:        any order of adding n numbers with one rounding to
//     nearest per addend errs by at most (n - 1) u sum|p| (1 + O(n u)); sum|p| <= (1 + 2^-8)^2 S, so <= 6.05 K u S.
//     The mainloop takes them two terms to an MFMA: 3 K / 16 v_mfma_f32_16x16x32_bf16 per element, each the sum of 32
//     products and C, and one of the three mixes ah bh with am bm, 2^-16 of its size.  What the instruction does
//     inside is not documented; measured (tools/mfma_bf16_probe.hip, its 16x16x32 part: 20 000 sums of 32 products
//     whose halves differ by 2^-16 or not at all, C zero, small or a running sum of up to 2^7): it is neither the exact
//     sum rounded once nor two 16-product steps rounded to nearest; with the smaller half in k 0..15, as here, it errs
//     by at most 2.7 u (|c| + sum|p|) per MFMA -> 0.51 K u (S + max|c|) (3.0 u with the smaller half in k 16..31,
//     and over the whole GEMM the rms error is 0.3 % larger that way round)
//   * the epilogue's one rounding of C += (accumulate)           (as in the fp32 tier)
// against the fp32 tier's k-ordered fmaf chain, K u S.  For uniform [-1, 1) data S ~ K / 4 and the errors add like a
// random walk; measured ratios of the two tiers' max errors are in profiles/gemm_bf16_split_notes.md.
//
// THE WINDOW.  The above needs no piece to be a bf16 subnormal (the matrix pipe may flush them), no product to
// underflow and no partial sum to overflow.  The cut passes check every element: it must be zero or satisfy
//     2^-40 <= |v| < 2^40.
//   * pieces: a nonzero piece of v in [2^e, 2^(e+1)) is a multiple of ulp(v) = 2^(e-23) >= 2^-63, far above bf16's
//     smallest normal 2^-126 (bf16 has fp32's exponent range);
//   * products: nonzero piece products are multiples of 2^-63 2^-63 = 2^-126, fp32's smallest normal, and so is any
//     sum of them: neither a product nor a partial sum is ever a nonzero subnormal;
//   * overflow: |pieces| <= 2^40 (1 + 2^-8), the six products of one k sum to < 1.02 2^80 in magnitude, and K < 2^31 of
//     them to < 2^112 < 2^128.
// An element outside the window -- or a NaN / Inf -- ORs a device flag.  The mainloop kernel returns at once when the
// flag is set, and a gated launch of the fp32 kernel (sp_gemm_f32_gated_kernel: the body of sp_gemm_glds_kernel) that
// follows it returns at once when it is clear: stream-ordered, no host wait, and such inputs get the fp32 tier's bits.
//
// IMAGES.  One pass per operand writes its three bf16 images k-tile-major, [K / 16][rows][16] (the layout
// sp_split_rows_kernel in kmeans_split.hpp documents: the k-tile of the rows a workgroup brings per k-step is one
// contiguous block), K padded to 16 with zeros.  A [M][K] is cut as it lies; B [K][N] must be k-contiguous per column,
// so its pass transposes a 16 x 256 block through LDS.  sp_gemm_ws keeps nothing between calls: every call cuts its
// operands into its workspace.  A caller that multiplies the same operand again cuts it once into a buffer of its own
// (sp_gemm_cut) and hands that to sp_gemm_ws_images; the images, the mainloop and so the bits are the same either way.
// Shapes whose images would not fit under GS_IMAGE_CAP stay on the fp32 tier (cutting K into slabs that accumulate
// into C is not built: 32768^3 would need seven).
//
// MAINLOOP (sp_gemm_glds_kernel_bf16x3).  256 x 256 workgroup tile, one workgroup per CU, 2 x 2 waves of 128 x 128
// each, one per SIMD with all 512 registers: the 8 x 8 accumulator blocks of 16 x 16 fill the 256 AGPRs, the
// fragments live in VGPRs.  Tiles are handed out by a walk of the kernel's own (sp_gemm_split_tile_of_block; the fp32
// kernels keep sp_gemm_tile_of_block and GROUP_M, fitted to 256 x 128 tiles, two workgroups per CU and row-major A).
// A workgroup loads one A panel and one B panel per k-tile, 24 KiB each, and the 32 workgroups resident on an XCD run
// in step, so what that XCD's L2 fetches from beyond it per k-tile is the DISTINCT tile rows plus tile columns among
// its 32 tiles: measured (2 x FETCH_SIZE, 8192^3) 13.29 / 7.25 / 4.83 / 4.83 / 7.25 GB per launch for windows of
// 1 x 32 / 2 x 16 / 4 x 8 / 8 x 4 / 16 x 2 tiles, which is 33 / 18 / 12 / 12 / 18 panels x 24 KiB x 512 k-tiles x 32
// windows to the last digit -- the model with no drift in k at all.  So the window is 4 x 8 (no 32 tiles touch fewer
// than 12 panels), m-fastest inside.  Across XCDs the eight windows of a round of 256 workgroups tile one 16 x 16
// rectangle of tiles, so that a round asks the fabric for 16 + 16 distinct panels, each from two or four XCDs, and not,
// as with a contiguous range of the tile order per XCD, for 32 + 8 with all eight XCDs on the same 8 B panels at
// once: same L2 traffic, 0.7 % less time on the headline, and the only arrangement that clears the project's bar
// (profiles/gemm_split_tile_walk_notes.md).  No workgroup waits for another: the walk is a function of the block id.
// k-tiles of 16 are brought by global_load_lds_dwordx4 into two LDS stages.  The MFMA is
// v_mfma_f32_16x16x32_bf16 (under this loop the chip holds a higher clock on it than on 32x32x16: measured in
// profiles/gemm_split_mfma_shape_notes.md), whose 32 k carry TWO terms of the same 16 k: lanes 0-31 of an operand
// (k-groups 0, 1) hold the 16 k of one image, lanes 32-63 (k-groups 2, 3) the same 16 k of another.  Three MFMAs per
// block and k-tile take the six products, smallest first, and inside an MFMA the smaller term first:
//     Pa = A [l | h] . B [h | l] = al bh + ah bl,   Pb = A [m | h] . B [h | m] = am bh + ah bm,
//     Pc = A [m | h] . B [m | h] = am bm + ah bh
// -- two variants of every A block and three of every B block, 40 ds_read_b128 and 192 MFMAs per wave and k-tile.
// The loop is software-pipelined one k-tile ahead IN REGISTERS: the MFMAs of k-tile t take every operand from VGPRs
// that were filled during k-tile t - 1, so no LDS latency stands between the barrier and the first MFMA.  During
// k-tile t a wave
//   * issues the 192 MFMAs of tile t, Pa, Pb, Pc each over the 8 x 8 blocks;
//   * reads the 40 fragments of tile t + 1 from stage (t + 1) & 1, one after every fourth MFMA: under Pa the A [m | h]
//     and B [m | h] of Pc into a second register set (they are live to the last MFMA), under Pb the operands of Pa
//     in place, under Pc the B [h | m] of Pb in place; the last read stands 35 MFMAs before the end;
//   * issues its 12 pieces of tile t + 2 into stage t & 1, one after every eighth MFMA of the first half;
// then waits for its pieces (vmcnt) AND its fragment reads (lgkmcnt) and meets the others at the one barrier per
// k-tile.  That barrier publishes tile t + 2 and tells every wave that stage (t + 1) & 1 has been read, so the pieces
// of tile t + 3 may overwrite it.  The loop is unrolled by two so that stages and register sets are constants.
// Every gap between two MFMAs is written to an ISSUE BUDGET of 16 cycles, the MFMA's own 8 included (by the issue
// prices measured for MI355X: costs add, and a gap runs max(16, their sum); the prices are not re-measured here, the
// kernel's cycles are), so a gap holds the MFMA and at most one of: a fragment read; a piece's load, alone;
// that piece's write of M0 (one s_add_u32 of a constant to the wave's LDS base), one gap EARLIER, so that the MFMA
// between them is the wait state the load needs behind it; the advance of one image's running 64-bit base by a slab
// (s_add_u32 / s_addc_u32), two gaps behind the image's last piece.  There is no multiply, no clamp and no other
// scalar work in the body, and nothing between the barrier and the next MFMA but the trip count of the two-k-tile
// loop.  The clamp min(t + 2, KT - 1) of the requested k-tile is in the code's shape instead: the loop runs k-tiles
// 0 .. KT - 3, and the last two are copies of the body whose bases stand on the last k-tile and do not advance -- they
// request it again, and the last one reads fragments nothing takes, both inside the images and the stages, so no
// body has a branch.  Reads and MFMAs are asm with tied destinations (see GS_READ_A, GS_MFMA).
// Measured and not kept (profiles/gemm_split_issue_budget_notes.md): an epilogue whose interior tiles store without a
// predicate and whose `accumulate` copy loads eight values per wait (no gain beyond the run-to-run spread, on the
// headline or on the K-split rows), and one persistent workgroup per CU whose last two k-tiles request the first two
// of its next tile (slower).
// An LDS image is [row][2 chunks of 16 B]; chunk q of row r lives in slot q ^ ((r >> 4) & 1).  A fragment read takes
// rows 16 blk .. 16 blk + 15 of one image in lanes 0-31 and of another in lanes 32-63, lane l chunk (l >> 4) & 1.  A
// ds_read_b128 is served in lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}: each takes rows {0-3, 12-15} at
// one chunk and rows {4-11} at the other, 8 distinct rows mod 8 at each of the two slots, which are the 16 distinct
// 16-byte units of the 256-byte bank period: conflict-free (SQ_LDS_BANK_CONFLICT = 0).
#pragma once
#include <utility>

typedef __bf16 gs_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gs_bf16x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GS_BK = 16;                         // k per k-tile
constexpr int GS_RB = GS_BK * 2;                  // bytes of a row of a k-tile of one image
constexpr unsigned GS_WIN_LO = (127u - 40u) << 23;   // bits of 2^-40
constexpr unsigned GS_WIN_HI = (127u + 40u) << 23;   // bits of 2^40
constexpr size_t GS_IMAGE_CAP = (size_t)2 << 30;  // bytes of operand images the tier may ask the workspace pool for
constexpr size_t GS_WS_HEAD = 512;                // the flag, and room to align what follows

struct GsCfg {
  static constexpr int BM = 256, BN = 256, NW = 4, THREADS = 64 * NW;   // 2 x 2 waves of 128 x 128
  static constexpr int A_BYTES = BM * GS_RB, B_BYTES = BN * GS_RB;      // one image of a k-tile
  static constexpr int STAGE_BYTES = 3 * A_BYTES + 3 * B_BYTES;         // Ah | Am | Al | Bh | Bm | Bl
  static constexpr int SMEM_BYTES = 2 * STAGE_BYTES;
  static constexpr int APW = A_BYTES / 1024 / NW, BPW = B_BYTES / 1024 / NW;   // 1-KiB pieces per wave and image
  static constexpr int NPIECES = 3 * APW + 3 * BPW;
  static constexpr int SLOTS = SP_CUS;                                  // resident workgroups
  static constexpr int NMFMA = 3 * 8 * 8;                               // per wave and k-tile
  static_assert(APW >= 1 && BPW >= 1 && APW * NW * 1024 == A_BYTES && BPW * NW * 1024 == B_BYTES, "tile / waves mismatch");
  static_assert(NPIECES * 8 <= NMFMA / 2, "one piece after every eighth MFMA of the first half");
  static_assert(STAGE_BYTES + 7 * 16 * GS_RB < 65536, "stage and block go into a ds_read's 16-bit offset");
};

// ---- the walk: block id -> tile of the mainloop (see MAINLOOP above) --------------------------------------------------
constexpr int GS_WALK_RH = 4;                     // tile rows of an XCD's window of 32 resident tiles; its columns: 32 / RH
constexpr int GS_WALK_SUPER = 16;                 // tile rows and columns of the rectangle the eight windows of a round tile
constexpr int GS_WALK_ROUND = 8 * 32;             // workgroups resident at once: 8 XCDs x 32 CUs
static_assert(32 % GS_WALK_RH == 0 && GS_WALK_SUPER % GS_WALK_RH == 0 &&
              GS_WALK_SUPER * GS_WALK_SUPER == GS_WALK_ROUND, "eight RH x 32 / RH windows tile the super-rectangle");

// A bijection from block ids onto tiles for every grid and block count nblk = tiles_m * tiles_n (tiles_m, tiles_n <=
// 2^23, what M, N < 2^31 give; tests/test_gemm_split_walk.py).  Position p of a block in THE ORDER: blocks bid, bid + 8,
// .. run on one XCD, so in a full round of 256 XCD x takes positions 32 x .. 32 x + 31 of the round; the blocks behind
// the last full round share out what is left in contiguous ranges, as sp_gemm_tile_of_block does.  THE ORDER itself:
// bands of SUPER tile rows; in a band, rectangles of SUPER tile columns; in a rectangle, strips of RH tile rows; in a
// strip, m-fastest -- each level clipped at the grid's edge, so every level holds whole numbers of the next one.
__host__ __device__ __forceinline__ void sp_gemm_split_tile_of_block(int bid, int nblk, int tiles_m, int tiles_n,
                                                                     int& tm, int& tn) {
  constexpr int S = GS_WALK_SUPER, RH = GS_WALK_RH;
  const int xcd = bid & 7, local = bid >> 3;
  const int full = nblk & ~(GS_WALK_ROUND - 1);
  int p;
  if (bid < full) {
    p = (local >> 5) * GS_WALK_ROUND + xcd * 32 + (local & 31);
  } else {
    const int rest = nblk - full, q = rest >> 3, r = rest & 7;
    p = full + (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + ((bid - full) >> 3);
  }
  const int band = p / (S * tiles_n);
  const int h1 = (tiles_m - band * S) < S ? (tiles_m - band * S) : S;           // the band's tile rows
  int q = p - band * S * tiles_n;
  const int rect = q / (h1 * S);
  const int w2 = (tiles_n - rect * S) < S ? (tiles_n - rect * S) : S;           // the rectangle's tile columns
  q -= rect * h1 * S;
  const int strip = q / (RH * w2);
  const int h3 = (h1 - strip * RH) < RH ? (h1 - strip * RH) : RH;               // the strip's tile rows
  q -= strip * RH * w2;
  tm = band * S + strip * RH + q % h3;
  tn = rect * S + q / h3;
}

template <int V>
struct GsInt {                                    // a constant handed to a generic lambda
  static constexpr int value = V;
};

template <int... I, typename F>
__device__ __forceinline__ void gs_unrolled(std::integer_sequence<int, I...>, F&& f) {   // f(GsInt<0>), f(GsInt<1>), ...
  (f(GsInt<I>{}), ...);
}

__device__ __forceinline__ bool gs_outside(float v) {
  const unsigned b = __float_as_uint(v) & 0x7fffffffu;
  return b != 0u && (b < GS_WIN_LO || b >= GS_WIN_HI);      // (NaN and Inf lie above GS_WIN_HI)
}

__device__ __forceinline__ void gs_cut(float v, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)v;
  const float r1 = v - (float)h;
  m = (__bf16)r1;
  l = (__bf16)(r1 - (float)m);
}

__device__ __forceinline__ void gs_raise(bool bad, unsigned* flag) {
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// Images of A [M][K]: [KT][M][16] each, `img` apart.  A lane takes 4 consecutive k of one row;
// 8 lanes a row's 32 k (two k-tiles), a wave 8 rows, a workgroup 32 rows x 256 k.
__global__ __launch_bounds__(256) void sp_gemm_cut_rows_kernel(const float* __restrict__ A, int64_t lda, int M, int K,
                                                               __bf16* __restrict__ Ah, int64_t img,
                                                               unsigned* __restrict__ flag) {
  const int q = threadIdx.x & 7, row = blockIdx.x * 32 + (threadIdx.x >> 3);
  const int kpad = (K + GS_BK - 1) / GS_BK * GS_BK;
  bool bad = false;
  if (row < M) {
    const float* __restrict__ a = A + (int64_t)row * lda;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int k = blockIdx.y * 256 + it * 32 + 4 * q;
      if (k >= kpad) break;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k + 4 <= K) {
        v = *(const f32x4*)(a + k);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < K) v[e] = a[k + e];
      }
      gs_bf16x4 h, m, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bad |= gs_outside(v[e]);
        __bf16 hh, mm, ll;
        gs_cut(v[e], hh, mm, ll);
        h[e] = hh;
        m[e] = mm;
        l[e] = ll;
      }
      const int64_t at = ((int64_t)(k >> 4) * M + row) * GS_BK + (k & 15);
      *(gs_bf16x4*)(Ah + at) = h;
      *(gs_bf16x4*)(Ah + img + at) = m;
      *(gs_bf16x4*)(Ah + 2 * img + at) = l;
    }
  }
  gs_raise(bad, flag);
}

// Images of B [K][N]: [KT][N][16] each.  A workgroup takes one k-tile of 256 columns: lane = column,
// 16 loads down k (a wave reads 256 B of a row per load), the three 32-byte image rows of its column through LDS, and
// the 8 KiB of each image go out as they lie there, 16 B per lane.
__global__ __launch_bounds__(256) void sp_gemm_cut_cols_kernel(const float* __restrict__ B, int64_t ldb, int N, int K,
                                                               __bf16* __restrict__ Bh, int64_t img,
                                                               unsigned* __restrict__ flag) {
  __shared__ __attribute__((aligned(16))) __bf16 s[3][256 * GS_BK];
  const int n0 = blockIdx.x * 256, col = n0 + threadIdx.x, k0 = blockIdx.y * GS_BK;
  float v[GS_BK];
#pragma unroll
  for (int e = 0; e < GS_BK; ++e) v[e] = (col < N && k0 + e < K) ? B[(int64_t)(k0 + e) * ldb + col] : 0.f;
  bool bad = false;
  gs_bf16x8 h[2], m[2], l[2];
#pragma unroll
  for (int e = 0; e < GS_BK; ++e) {
    bad |= gs_outside(v[e]);
    __bf16 hh, mm, ll;
    gs_cut(v[e], hh, mm, ll);
    h[e >> 3][e & 7] = hh;
    m[e >> 3][e & 7] = mm;
    l[e >> 3][e & 7] = ll;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    *(gs_bf16x8*)(&s[0][threadIdx.x * GS_BK + 8 * c]) = h[c];
    *(gs_bf16x8*)(&s[1][threadIdx.x * GS_BK + 8 * c]) = m[c];
    *(gs_bf16x8*)(&s[2][threadIdx.x * GS_BK + 8 * c]) = l[c];
  }
  __syncthreads();
  const int64_t base = ((int64_t)blockIdx.y * N + n0) * GS_BK;
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int at = (c * 256 + threadIdx.x) * 8;            // element of the 256 x 16 block; its row: at / 16
      if (n0 + at / GS_BK < N) *(gs_bf16x8*)(Bh + p * img + base + at) = *(const gs_bf16x8*)(&s[p][at]);
    }
  gs_raise(bad, flag);
}

// The mainloop.  Ah / Bh: the hi images, mid and lo `a_img` / `b_img` BYTES behind; KT k-tiles, `a_slab` / `b_slab` bytes
// apart in an image: 32 x the rows the image was cut with, which is M / N, or more when Ah / Bh point at a row block of
// the images of a larger operand.  flag_a / flag_b: the window flag of either operand's cut (they may be one word).
__global__ __launch_bounds__(GsCfg::THREADS, 1) void sp_gemm_glds_kernel_bf16x3(
    const char* __restrict__ Ah, int64_t a_img, const char* __restrict__ Bh, int64_t b_img, float* __restrict__ C,
    int64_t ldc, int M, int N, int KT, int accumulate, int tiles_m, int tiles_n, int64_t a_slab, int64_t b_slab,
    const unsigned* __restrict__ flag_a, const unsigned* __restrict__ flag_b) {
  using G = GsCfg;
  constexpr int APW = G::APW, BPW = G::BPW, NPIECES = G::NPIECES;
  static_assert(APW == BPW, "the six images of a request take the same number of pieces");
  constexpr int PW = APW;
  extern __shared__ __attribute__((aligned(16))) char gs_smem[];
  if ((*flag_a | *flag_b) != 0u) return;                     // an operand left the window: the gated fp32 launch computes C
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;                     // wm: which 128 rows, wn: which 128 columns
  const int l15 = lane & 15, lq = lane >> 4;                 // an operand's row / a result's column, and the k-group

  // ---- k-tile pieces: 1 KiB = one wave-wide 16-B load = 32 rows of one image; rows past the operand's end repeat
  // its last row (their results are masked on store)
  auto piece_offsets = [&](int r0, int rows, unsigned (&off)[PW]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int slot = (wid * PW + j) * 64 + lane;
      int row = slot >> 1;
      const int q = (slot & 1) ^ ((row >> 4) & 1);
      if (r0 + row > rows - 1) row = rows - 1 - r0;
      off[j] = (unsigned)(row * GS_RB + q * 16);
    }
  };
  const unsigned s_base = SP_LDS_ADDR(gs_smem);

  // A request is 12 pieces: image i / PW of A, then of B.  Piece i goes out in two asm statements, in two MFMA gaps:
  // GS_PIECE_M0 writes its LDS target to M0, GS_PIECE_LOAD is the load, and the MFMA between them is the wait state
  // an LDS-DMA needs behind a write of M0.  `asm volatile` keeps them in order and the write names M0 as clobbered;
  // the load's use of M0 cannot be stated, so nothing the compiler generates between the two may write M0 (none does:
  // read in the ISA of the loop and the prologue), and this kernel must not use the global_load_lds builtin.  M0 is
  // the wave's first piece of stage 0 plus a constant, in one s_add_u32: a table of the 24 targets would take 24 SGPRs.
  const unsigned s_wave = s_base + (unsigned)(wid * PW) * 1024u;
#define GS_PIECE_LDS(stage_, i) \
  ((stage_) * G::STAGE_BYTES + ((i) < 3 * PW ? 0 : 3 * G::A_BYTES) + (((i) / PW) % 3) * G::A_BYTES + ((i) % PW) * 1024)
#define GS_PIECE_M0(stage_, i) \
  asm volatile("s_add_u32 m0, %0, %1" ::"s"(s_wave), "n"(GS_PIECE_LDS(stage_, i)) : "memory", "scc", "m0")
#define GS_PIECE_LOAD(base, voff) asm volatile("global_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base) : "memory")
  static_assert(G::A_BYTES == G::B_BYTES, "GS_PIECE_LDS strides both operands' images by A_BYTES");

  // The accumulators: 16 x 16 blocks, col = l15, row = 4 lq + r; 256 registers, all of the AGPRs.  The MFMA is asm with
  // the accumulator tied ("+a"): left to the builtin, hipcc's allocator rotated the blocks through the AGPRs from MFMA
  // to MFMA and spilled 940 registers.  What the compiler then no longer sees is the MFMA's latency, so the waits it
  // would have inserted are stated: an accumulator is taken again 64 MFMAs later, GS_ACC_ZEROED puts the zeros in
  // place before a tile's first fragment reads, and GS_ACC_DONE stands between the last MFMAs and the epilogue.
  f32x4 acc[8][8];
#define GS_MFMA(c, a, b) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b))
#define GS_ACC_ZEROED(c) asm volatile("" : "+a"(c))
#define GS_ACC_DONE(x)                                                                                              \
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3"                                                                      \
               : "+a"(x[0]), "+a"(x[1]), "+a"(x[2]), "+a"(x[3]), "+a"(x[4]), "+a"(x[5]), "+a"(x[6]), "+a"(x[7]))

  // A fragment is an operand of a 16x16x32 MFMA that carries two terms: k-groups 0, 1 (lanes 0-31) are the 16 k of one
  // image, k-groups 2, 3 (lanes 32-63) the same 16 k of another.  Lane l reads row 16 blk + l15 of its image, chunk
  // (lq & 1), which lies in slot (lq & 1) ^ (blk & 1).  One base register per variant and block parity; the stage and
  // the block go into the read's offset.  Variants (image of lanes 0-31 | of lanes 32-63; 0 hi, 1 mid, 2 lo):
  //   A: 0 = [l | h], 1 = [m | h];   B: 0 = [h | l], 1 = [h | m], 2 = [m | h]
  const int up = lane >> 5;
  unsigned a_rd[2][2], b_rd[3][2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const unsigned a_row = s_base + (unsigned)((wm * 128 + l15) * GS_RB + (((lq & 1) ^ par) * 16));
    const unsigned b_row = s_base + (unsigned)(3 * G::A_BYTES + (wn * 128 + l15) * GS_RB + (((lq & 1) ^ par) * 16));
    a_rd[0][par] = a_row + (unsigned)((up ? 0 : 2) * G::A_BYTES);
    a_rd[1][par] = a_row + (unsigned)((up ? 0 : 1) * G::A_BYTES);
    b_rd[0][par] = b_row + (unsigned)((up ? 2 : 0) * G::B_BYTES);
    b_rd[1][par] = b_row + (unsigned)((up ? 1 : 0) * G::B_BYTES);
    b_rd[2][par] = b_row + (unsigned)((up ? 0 : 1) * G::B_BYTES);
  }

  // The fragments of k-tile t.  a_lh, b_hl and b_hm are one set of registers, which tile t + 1 refills once the term
  // that takes them is through; a_mh and b_mh are live to the last MFMA, so they have two sets and tile t uses set
  // t & 1.
  gs_bf16x8 a_lh[8], b_hl[8], b_hm[8], a_mh[2][8], b_mh[2][8];
  // A fragment read, variant v_ of stage s_, block blk_, into `dst`.  Written in asm with the destination tied
  // ("+v"): the new fragment goes into the very registers of the old one, which hipcc's allocator does not find by
  // itself (it took fresh registers for the next tile and spilled).  The compiler then does not count these reads in
  // lgkmcnt, so GS_READS_DONE states the wait, and passes every fragment through it: no MFMA that takes one can be
  // moved in front of the wait.
#define GS_READ_A(dst, s_, v_, blk_)                                       \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(dst) : "v"(a_rd[v_][(blk_) & 1]), \
               "n"((s_) * G::STAGE_BYTES + (blk_) * 16 * GS_RB) : "memory")
#define GS_READ_B(dst, s_, v_, blk_)                                       \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "+v"(dst) : "v"(b_rd[v_][(blk_) & 1]), \
               "n"((s_) * G::STAGE_BYTES + (blk_) * 16 * GS_RB) : "memory")
  // (a tile's first fill: nothing is in the registers yet, so the destination is an output only, and the set the
  // first k-tile refills is merely declared written)
#define GS_FILL_A(dst, v_, blk_) \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(a_rd[v_][(blk_) & 1]), "n"((blk_) * 16 * GS_RB) : "memory")
#define GS_FILL_B(dst, v_, blk_) \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(b_rd[v_][(blk_) & 1]), "n"((blk_) * 16 * GS_RB) : "memory")
#define GS_FILL_NONE(dst) asm volatile("" : "=v"(dst))
#define GS_TIE8(x) "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
#define GS_READS_DONE(s_)                                                                              \
  do {                                                                                                 \
    asm volatile("s_waitcnt lgkmcnt(0)" : GS_TIE8(a_lh), GS_TIE8(b_hl), GS_TIE8(b_hm) :: "memory");    \
    asm volatile("" : GS_TIE8(a_mh[s_]), GS_TIE8(b_mh[s_]) :: "memory");                               \
  } while (0)

  // One k-tile: its 192 MFMAs -- Pa = [l | h] [h | l], Pb = [m | h] [h | m], Pc = [m | h] [m | h], each over the 8 x 8
  // blocks of the wave -- from registers alone.  Every gap between two MFMAs has an issue budget of 16 cycles, 8 of
  // them the MFMA's own, and holds at most one of:
  //   * a fragment read of tile t + 1 from stage (t + 1) & 1, after every fourth MFMA: under Pa the 16 fragments Pc
  //     takes, into the other set; under Pb the 16 of Pa, in place; under Pc the 8 that only Pb takes, in place (the
  //     last one 35 MFMAs before the end);
  //   * a piece of the request into stage t & 1, after MFMA 8 i + 7 of the first half, and nothing else;
  //   * that piece's write of M0, one gap earlier;
  //   * the advance of an image's running base (one s_add_u32 / s_addc_u32), two gaps behind the image's last piece.
  // What is requested is the caller's: `pa` / `pb` are the running bases of the six images, at the k-tile to bring,
  // `oa` / `ob` the lanes' offsets, `ia` / `ib` what the bases advance by.  The steady body asks for k-tile t + 2 and
  // advances by a slab; the last two k-tiles ask for the last one again and stand still (below).  The body has no
  // branch, no multiply and no scalar work in front of its first MFMA.  `par` is t & 1 as a constant: stages and
  // register sets are then fixed per copy of the body, and nothing is moved between the sets.
  auto ktile = [&](auto par_, const char* (&pa)[3], const char* (&pb)[3], const unsigned (&oa)[PW],
                   const unsigned (&ob)[PW], int64_t ia, int64_t ib) __attribute__((always_inline)) {
    constexpr int CUR = decltype(par_)::value, NXT = CUR ^ 1;
    gs_unrolled(std::make_integer_sequence<int, G::NMFMA>{}, [&](auto idx_) __attribute__((always_inline)) {
      constexpr int idx = decltype(idx_)::value, term = idx >> 6, i = (idx >> 3) & 7, j = idx & 7;
      const gs_bf16x8 a = term == 0 ? a_lh[i] : a_mh[CUR][i];
      const gs_bf16x8 b = term == 0 ? b_hl[j] : term == 1 ? b_hm[j] : b_mh[CUR][j];
      GS_MFMA(acc[i][j], a, b);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr ((idx & 3) == 0) {
        constexpr int q = (idx & 63) >> 2, blk = q & 7;        // the 16 read gaps of a term
        if constexpr (term == 0 && q < 8) GS_READ_A(a_mh[NXT][blk], NXT, 1, blk);
        if constexpr (term == 0 && q >= 8) GS_READ_B(b_mh[NXT][blk], NXT, 2, blk);
        if constexpr (term == 1 && q < 8) GS_READ_A(a_lh[blk], NXT, 0, blk);        // a_lh, b_hl: free after Pa
        if constexpr (term == 1 && q >= 8) GS_READ_B(b_hl[blk], NXT, 0, blk);
        if constexpr (term == 2 && q < 8) GS_READ_B(b_hm[blk], NXT, 1, blk);        // b_hm: after Pb
      }
      if constexpr (idx % 8 == 6 && idx / 8 < NPIECES) GS_PIECE_M0(CUR, idx / 8);
      if constexpr (idx % 8 == 7 && idx / 8 < NPIECES) {
        constexpr int pc = idx / 8, img = pc / PW;
        if constexpr (img < 3) GS_PIECE_LOAD(pa[img], oa[pc % PW]);
        else GS_PIECE_LOAD(pb[img - 3], ob[pc % PW]);
      }
      if constexpr (idx % (8 * PW) == 1 && idx / (8 * PW) >= 1 && idx / (8 * PW) <= 6) {
        constexpr int img = idx / (8 * PW) - 1;
        if constexpr (img < 3) {
          pa[img] += ia;
          asm volatile("" : "+s"(pa[img]));
        } else {
          pb[img - 3] += ib;
          asm volatile("" : "+s"(pb[img - 3]));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    SP_GLDS_LANDED();
    GS_READS_DONE(NXT);
    // the request has landed in stage t & 1, and this wave's reads of stage (t + 1) & 1 have returned, before any
    // wave's next pieces may overwrite it
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  };
  GsInt<0> even;
  GsInt<1> odd;

  // ---- the tile.  Written once and instantiated per parity of the count of k-tiles, prologue and epilogue included:
  // with both sequences of bodies behind one loop, or with the two paths joined again in front of one epilogue, hipcc's
  // allocator has to reconcile two assignments of the 480 live registers and spills (3652 and 754 VGPRs).
  auto tile = [&](auto odd_count_) __attribute__((always_inline)) {
    constexpr bool ODD = decltype(odd_count_)::value != 0;
    int tm, tn;
    sp_gemm_split_tile_of_block(blockIdx.x, gridDim.x, tiles_m, tiles_n, tm, tn);
    const int m0 = tm * G::BM, n0 = tn * G::BN;
    unsigned a_off[PW], b_off[PW];
    piece_offsets(m0, M, a_off);
    piece_offsets(n0, N, b_off);
    const char *ra[3], *rb[3];                               // the images' running bases, at the k-tile to request
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      ra[p] = Ah + (int64_t)m0 * GS_RB + p * a_img;
      rb[p] = Bh + (int64_t)n0 * GS_RB + p * b_img;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        GS_ACC_ZEROED(acc[i][j]);
      }
    // prologue: k-tile 0 lands and is published; k-tile 1's request goes out whole; k-tile 0's fragments are read
    gs_unrolled(std::make_integer_sequence<int, 2 * NPIECES>{}, [&](auto n_) __attribute__((always_inline)) {
      constexpr int s = decltype(n_)::value / NPIECES, i = decltype(n_)::value % NPIECES;
      GS_PIECE_M0(s, i);
      asm volatile("s_nop 0");                               // (no MFMA stands between the two here)
      if constexpr (i < 3 * PW) GS_PIECE_LOAD(ra[i / PW], a_off[i % PW]);
      else GS_PIECE_LOAD(rb[i / PW - 3], b_off[i % PW]);
      if constexpr (i == NPIECES - 1) {
        if constexpr (s == 0) {
          SP_GLDS_LANDED();
          __syncthreads();
        }
        const int64_t da = s == 0 && KT < 2 ? 0 : a_slab, db = s == 0 && KT < 2 ? 0 : b_slab;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          ra[p] += da;                                       // (after both: k-tile 2, which only KT >= 3 requests)
          rb[p] += db;
        }
      }
    });
#pragma unroll
    for (int blk = 0; blk < 8; ++blk) {
      GS_FILL_A(a_lh[blk], 0, blk);
      GS_FILL_A(a_mh[0][blk], 1, blk);
      GS_FILL_B(b_hl[blk], 0, blk);
      GS_FILL_B(b_hm[blk], 1, blk);
      GS_FILL_B(b_mh[0][blk], 2, blk);
      GS_FILL_NONE(a_mh[1][blk]);
      GS_FILL_NONE(b_mh[1][blk]);
    }
    SP_GLDS_LANDED();
    GS_READS_DONE(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);

    // k-tiles 0 .. KT - 3 request k-tile t + 2 and step on by a slab, two per trip (and one more for an odd count);
    // the last two request the last k-tile once more, with no step: the clamp of t + 2 costs the loop nothing
    for (int n = (KT - 2) >> 1; n > 0; --n) {
      ktile(even, ra, rb, a_off, b_off, a_slab, b_slab);
      ktile(odd, ra, rb, a_off, b_off, a_slab, b_slab);
    }
    const auto last_ktile = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        ra[p] = Ah + (int64_t)m0 * GS_RB + p * a_img + (int64_t)(KT - 1) * a_slab;
        rb[p] = Bh + (int64_t)n0 * GS_RB + p * b_img + (int64_t)(KT - 1) * b_slab;
      }
    };
    if constexpr (ODD) {
      if (KT >= 3) {
        ktile(even, ra, rb, a_off, b_off, a_slab, b_slab);
        last_ktile();
        ktile(odd, ra, rb, a_off, b_off, 0, 0);
      } else {
        last_ktile();
      }
      ktile(even, ra, rb, a_off, b_off, 0, 0);
    } else {
      last_ktile();
      ktile(even, ra, rb, a_off, b_off, 0, 0);
      ktile(odd, ra, rb, a_off, b_off, 0, 0);
    }
    GS_ACC_DONE(acc[7]);                       // the last eight MFMAs wrote row 7; the pipe is in order, so all are through

    // ---- epilogue: C/D layout col = lane & 15, row = 4 (lane >> 4) + r.  A block alone writes 64-byte half-lines, so
    // blocks j and j + 1 of a row go out back to back: a row's 32 consecutive floats leave together.
    const int row0 = m0 + wm * 128 + 4 * lq, col0 = n0 + wn * 128 + l15;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int jp = 0; jp < 8; jp += 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + i * 16 + r;
#pragma unroll
          for (int j = jp; j < jp + 2; ++j) {
            const int col = col0 + j * 16;
            if (row < M && col < N) {
              float* p = C + (int64_t)row * ldc + col;
              float v;                       // (read where it is stored: hipcc otherwise copies all 256 at once and spills)
              asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(acc[i][j][r]));
              if (accumulate) v += *p;
              *p = v;
            }
          }
        }
      }
    }
  };
  if (KT & 1) tile(GsInt<1>{});
  else tile(GsInt<0>{});
#undef GS_MFMA
#undef GS_ACC_ZEROED
#undef GS_ACC_DONE
#undef GS_READ_A
#undef GS_READ_B
#undef GS_FILL_A
#undef GS_FILL_B
#undef GS_FILL_NONE
#undef GS_READS_DONE
#undef GS_TIE8
#undef GS_PIECE_LDS
#undef GS_PIECE_M0
#undef GS_PIECE_LOAD
}

// The fp32 kernel behind the flag: sp_gemm_glds_kernel's body, run only when an operand left the window.
template <typename Cfg, int BM, int BN, int WM, int WN, int WGS>
__global__ __launch_bounds__(Cfg::THREADS, WGS) void sp_gemm_f32_gated_kernel(
    const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb, float* __restrict__ C,
    int64_t ldc, int M, int N, int K, int accumulate, int tiles_m, int tiles_n, const unsigned* __restrict__ flag_a,
    const unsigned* __restrict__ flag_b) {
  if ((*flag_a | *flag_b) == 0u) return;
  sp_gemm_glds_body<Cfg, BM, BN, WM, WN>(A, lda, B, ldb, C, ldc, M, N, K, accumulate, tiles_m, tiles_n);
}

// ---- plan ---------------------------------------------------------------------------------------------------------
// Whether the tier is taken.  It is where the fp32 tier would run the data-parallel 256 x 128 direct-to-LDS kernel (so
// that the gated fallback reproduces it bit for bit) on at least one full round of tiles, the images fit under
// GS_IMAGE_CAP, and a cost model says the cut passes are amortised: the cut moves 10 bytes per operand element at the
// streaming rate, and the mainloop runs ceil(tiles / slots) rounds of 6 bf16 products at the rate the k-means split
// kernel sustains (1.1e15 issued flop/s); the fp32 tier is priced as in sp_sk_plan.
// SP_GEMM_SPLIT=0 (read once) keeps the fp32 tier everywhere.
#define GS_CUT_BYTES_PER_S 3.0e12
#define GS_ISSUED_FLOPS 1.1e15
static bool sp_gemm_bf16_plan(int64_t M, int64_t N, int64_t K) {
  static int mode = -2;
  if (mode == -2) {
    const char* e = getenv("SP_GEMM_SPLIT");
    mode = e ? atoi(e) : 1;
  }
  using G = GsCfg;
  if (mode == 0 || K < 16 || N % 4 != 0 || N < 4 || M < 1 || M > 2147483647LL || N > 2147483647LL || K > 2147483647LL)
    return false;
  const int64_t tb = ((M + 255) / 256) * ((N + 127) / 128);
  if (tb < 2 * SP_CUS || tb >= 2147483647LL) return false;    // the 256 x 128 tiles do not fill the chip
  double dp_cost;
  if (sp_gemm_dp_choice(M, N, &dp_cost) != 6 || sp_sk_plan(M, N, K)) return false;
  const int64_t KT = (K + GS_BK - 1) / GS_BK;
  if ((double)KT * 3.0 * GS_RB * ((double)M + (double)N) > (double)GS_IMAGE_CAP) return false;
  const double fp32_s = dp_cost * 128.0 * 128.0 * (double)K * 2.0 / (157.3e12 * 0.95 / SP_CUS);
  const int64_t tiles = ((M + G::BM - 1) / G::BM) * ((N + G::BN - 1) / G::BN);
  const int64_t rounds = (tiles + G::SLOTS - 1) / G::SLOTS;
  const double main_s = (double)rounds * G::SLOTS * (6.0 * 2.0 * G::BM * G::BN * (double)K) / GS_ISSUED_FLOPS;
  const double cut_s = 10.0 * ((double)M + (double)N) * (double)K / GS_CUT_BYTES_PER_S;
  return (main_s + cut_s + 20e-6) < 0.92 * fp32_s;
}

static size_t sp_gemm_bf16_ws_bytes(int64_t M, int64_t N, int64_t K) {
  return GS_WS_HEAD + (size_t)((K + GS_BK - 1) / GS_BK) * 3 * GS_RB * (size_t)(M + N);
}

// ---- one operand's images -----------------------------------------------------------------------------------------
// An image buffer: a 256-byte head whose first word is the operand's own window flag, then the three images
// [ceil(K / 16)][rows][16] bf16.  The workspace of a call that cuts its operands itself holds the same thing twice over:
// one head (both cuts raise its one flag), A's images, B's images.
constexpr size_t GS_IMG_HEAD = 256;

static size_t sp_gemm_bf16_image_bytes(int64_t rows, int64_t K) {
  return GS_IMG_HEAD + (size_t)((K + GS_BK - 1) / GS_BK) * 3 * GS_RB * (size_t)rows;
}

static long long gs_cut_launches = 0;      // cut kernels launched by this process (sp_gemm_cut_launches: what the tests count)

// Cut X (side 0: A [rows][K]; side 1: B [K][rows]) into the images at `img`, `img_stride` bytes apart, raising `flag`.
static void sp_gemm_bf16_cut(int side, const float* X, int64_t ld, int64_t rows, int64_t K, char* img, unsigned* flag,
                             hipStream_t st) {
  const int64_t KT = (K + GS_BK - 1) / GS_BK;
  const int64_t img_stride = KT * rows * GS_RB;                        // bytes
  __atomic_add_fetch(&gs_cut_launches, 1, __ATOMIC_RELAXED);
  if (side == 0)
    hipLaunchKernelGGL(sp_gemm_cut_rows_kernel, dim3((unsigned)((rows + 31) / 32), (unsigned)((K + 255) / 256)), dim3(256), 0,
                       st, X, ld, (int)rows, (int)K, (__bf16*)img, img_stride / 2, flag);
  else
    hipLaunchKernelGGL(sp_gemm_cut_cols_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)KT), dim3(256), 0, st, X, ld,
                       (int)rows, (int)K, (__bf16*)img, img_stride / 2, flag);
}

// The multiply.  imgA / imgB: an operand's image buffer (head first) cut with a_rows / b_rows rows, of which this
// product takes rows [a_row0, a_row0 + M) / [b_row0, b_row0 + N) -- or null: that operand is cut into `ws` here.
static int sp_gemm_bf16_launch(const float* A, int64_t lda, const char* imgA, int64_t a_rows, int64_t a_row0,
                               const float* B, int64_t ldb, const char* imgB, int64_t b_rows, int64_t b_row0, float* C,
                               int64_t ldc, int64_t M, int64_t N, int64_t K, int acc, void* ws, hipStream_t st) {
  using G = GsCfg;
  const int64_t KT = (K + GS_BK - 1) / GS_BK;
  const int64_t tiles_m = (M + G::BM - 1) / G::BM, tiles_n = (N + G::BN - 1) / G::BN;
  auto kern = sp_gemm_glds_kernel_bf16x3;
  using FCfg = GldsCfg<256, 128, 2, 2>;
  auto gated = sp_gemm_f32_gated_kernel<FCfg, 256, 128, 2, 2, 2>;
  static bool attr_set = false;
  if (!attr_set) {
    SP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G::SMEM_BYTES));
    SP_HIP(hipFuncSetAttribute((const void*)gated, hipFuncAttributeMaxDynamicSharedMemorySize, FCfg::LDS_BYTES));
    attr_set = true;
  }
  char* base = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);      // (not touched when both operands come cut)
  char* next = base + GS_IMG_HEAD;
  if (!imgA || !imgB) SP_HIP(hipMemsetAsync(base, 0, GS_IMG_HEAD, st));
  const unsigned* flag_a = (const unsigned*)(imgA ? imgA : base);
  const unsigned* flag_b = (const unsigned*)(imgB ? imgB : base);
  const char *Ah, *Bh;
  if (imgA) {
    Ah = imgA + GS_IMG_HEAD + a_row0 * GS_RB;
  } else {
    a_rows = M;
    sp_gemm_bf16_cut(0, A, lda, M, K, next, (unsigned*)base, st);
    Ah = next;
    next += 3 * KT * M * GS_RB;
  }
  if (imgB) {
    Bh = imgB + GS_IMG_HEAD + b_row0 * GS_RB;
  } else {
    b_rows = N;
    sp_gemm_bf16_cut(1, B, ldb, N, K, next, (unsigned*)base, st);
    Bh = next;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_m * tiles_n)), dim3(G::THREADS), G::SMEM_BYTES, st, Ah,
                     KT * a_rows * GS_RB, Bh, KT * b_rows * GS_RB, C, ldc, (int)M, (int)N, (int)KT, acc, (int)tiles_m,
                     (int)tiles_n, a_rows * GS_RB, b_rows * GS_RB, flag_a, flag_b);
  const int64_t ftm = (M + 255) / 256, ftn = (N + 127) / 128;
  hipLaunchKernelGGL(gated, dim3((unsigned)(ftm * ftn)), dim3(FCfg::THREADS), FCfg::LDS_BYTES, st, A, lda, B, ldb, C, ldc,
                     (int)M, (int)N, (int)K, acc, (int)ftm, (int)ftn, flag_a, flag_b);
  SP_CHECK_LAUNCH();
  return 0;
}

}  // namespace
