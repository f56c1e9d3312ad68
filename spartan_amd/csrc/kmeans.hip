// k-means tile kernels: the per-tile bodies of the reference's k-means mappers
// (spartan/examples/sklearn/cluster/k_means_.py):
//   kmeans_map2_dist_mapper / kmeans_outer_dist_mapper (:52-66)
//        labels = np.argmin(cdist(points, centers), axis=1)      -> sp_nearest_center
//   kmeans_count_mapper (:69-72)   np.bincount(labels, minlength=k) -> sp_bincount_i64
//   kmeans_center_mapper (:75-97)  new_centers[i] = points[labels == i].sum(axis=0)
//        (also _find_cluster_mapper :35-42)                       -> sp_segment_sum
//
// sp_nearest_center has two tiers (same results, see kmeans_mfma.hpp):
//   exact : one wavefront per point, squared distances accumulated in fp64 in
//           feature order exactly like cdist's C loop, sqrt, first-minimum;
//   fused : fp32 MFMA GEMM  x.c^T  with the argmin fused into the epilogue (the
//           n x k distance matrix is never written); points whose two best
//           scores are closer than the fp32 error bound are re-done by the exact
//           kernel, so the labels are those of the exact tier.
// sp_segment_sum adds the rows of each cluster sequentially in ascending row
// order (one lane per feature column), which is the order NumPy's axis-0 sum
// uses, after a stable counting sort of the row ids by label -- deterministic,
// no floating-point atomics.
#include "sp_common.hpp"

namespace {

// ------------------------------------------------------------------ exact tier
// Ct64[j][c] = (double)C[c][j], zero padded to [d][kp]: lanes (= centers) read it coalesced
template <typename TC>
__global__ __launch_bounds__(256) void sp_centers_t64_kernel(const TC* __restrict__ C, int64_t ldc, int k, int d,
                                                             int kp, double* __restrict__ Ct64) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [d][kp]
  if (i >= (int64_t)d * kp) return;
  const int j = (int)(i / kp), c = (int)(i - (int64_t)j * kp);
  Ct64[i] = c < k ? (double)C[(int64_t)c * ldc + j] : 0.0;
}

// One wavefront per R points.  Lane l owns centers l, l+64, ... (G at a time); each squared
// distance is accumulated over the features sequentially in fp64 and sqrt'ed -- cdist
// 'euclidean' on doubles, bit for bit -- then the wave takes the lexicographic
// (distance, index) minimum = np.argmin's first minimum.  Every center value loaded from
// the (L2-resident) Ct64 is used for the R points of the wave: the kernel is bound by
// L2 -> CU traffic otherwise.
// rows == NULL: every point 0..n-1; else the *n_rows points listed in rows[] (the ones the
// fused kernel could not decide) -- and only if there are MORE than `handled_elsewhere` of them
// (a shorter list is served by the candidate masks, sp_nearest_candidates_kernel).
template <typename TX>
__global__ __launch_bounds__(256) void sp_nearest_exact_kernel(const TX* __restrict__ X, int64_t ldx,
                                                               const double* __restrict__ Ct64, int kp, int64_t n,
                                                               int k, int d, int64_t* __restrict__ labels,
                                                               const int* __restrict__ rows,
                                                               const int* __restrict__ n_rows,
                                                               int64_t handled_elsewhere) {
  constexpr int G = 2, R = 8, J = 4;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t count = rows ? (int64_t)*n_rows : n;
  if (rows && count <= handled_elsewhere) return;
  for (int64_t it = wave * R; it < count; it += nwaves * R) {
    int64_t row[R];
    const TX* __restrict__ xr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t e = it + r < count ? it + r : count - 1;   // tail: repeat the last point
      row[r] = rows ? (int64_t)rows[e] : e;
      xr[r] = X + row[r] * ldx;
    }
    double best[R];
    int best_k[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      best[r] = INFINITY;
      best_k[r] = 0x7fffffff;
    }
    for (int c0 = 0; c0 < k; c0 += 64 * G) {
      double s[R][G];
      int col[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int c = c0 + g * 64 + lane;
        col[g] = c < kp ? c : kp - 1;   // (columns k..kp-1 are zero padding; beyond kp: clamp, result unused)
#pragma unroll
        for (int r = 0; r < R; ++r) s[r][g] = 0.0;
      }
      int j = 0;
      for (; j + J <= d; j += J) {
        double xv[R][J], cv[J][G];
#pragma unroll
        for (int u = 0; u < J; ++u) {
#pragma unroll
          for (int g = 0; g < G; ++g) cv[u][g] = Ct64[(int64_t)(j + u) * kp + col[g]];
#pragma unroll
          for (int r = 0; r < R; ++r) xv[r][u] = (double)xr[r][j + u];
        }
#pragma unroll
        for (int u = 0; u < J; ++u)   // feature order preserved within every chain
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const double diff = xv[r][u] - cv[u][g];
              s[r][g] += diff * diff;
            }
      }
      for (; j < d; ++j) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const double cvv = Ct64[(int64_t)j * kp + col[g]];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const double diff = (double)xr[r][j] - cvv;
            s[r][g] += diff * diff;
          }
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {   // ascending center index: `<` keeps the first minimum
        const int c = c0 + g * 64 + lane;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double v = sqrt(s[r][g]);
          if (c < k && v < best[r]) {
            best[r] = v;
            best_k[r] = c;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double b = best[r];
      int bk = best_k[r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(b, off);
        const int ok = __shfl_xor(bk, off);
        if (ob < b || (ob == b && ok < bk)) {
          b = ob;
          bk = ok;
        }
      }
      if (lane == 0) labels[row[r]] = bk == 0x7fffffff ? 0 : bk;
    }
  }
}

// Last step of the MFMA tiers: cdist's exact distance (sequential fp64 sum of squared differences in feature
// order, sqrt) of the centers the re-check pass marked for each listed point, and the lexicographic (distance,
// index) minimum = np.argmin's first minimum.
// SIXTEEN LANES PER LISTED POINT, ONE LANE PER CANDIDATE (round 4: a whole wavefront per point; before that a lane
// walked the set bits of one mask word one after the other, 91 - 256 us for 17 - 38 thousand points of configs[3]):
// the lanes of a group first write the numbers
// of the marked centers, in ascending order, into a list (a lane owns the mask words gl, gl + 16, ...; a scan
// of the popcounts over the group places them), then lane j runs the chain of candidate j -- the point's row is the same address for
// every lane, the center rows come straight from the caller's centers, both read J features ahead of the sum -- and a
// reduction over the group picks the minimum.  More than 16 candidates: 16 at a time.  A point with ONE candidate (its window
// holds the first pass's best only) is settled without reading a row; one with more than the list holds falls back to
// every lane walking its own mask words.
// cdist 'euclidean' of one (point, center) pair on doubles: the squared differences added in feature order, sqrt;
// the rows are read J features ahead of the sum
template <typename TC>
__device__ __forceinline__ double km_exact_distance(const float* __restrict__ xr, const TC* __restrict__ cr, int d) {
  constexpr int J = 8;
  double s = 0.0;
  int jj = 0;
  if (J <= d) {
    float xa[J];
    TC ca[J];
#pragma unroll
    for (int u = 0; u < J; ++u) {
      xa[u] = xr[u];
      ca[u] = cr[u];
    }
    for (; jj + 2 * J <= d; jj += J) {
      float xb[J];
      TC cb[J];
#pragma unroll
      for (int u = 0; u < J; ++u) {
        xb[u] = xr[jj + J + u];
        cb[u] = cr[jj + J + u];
      }
#pragma unroll
      for (int u = 0; u < J; ++u) {
        const double diff = (double)xa[u] - (double)ca[u];
        s += diff * diff;
      }
#pragma unroll
      for (int u = 0; u < J; ++u) {
        xa[u] = xb[u];
        ca[u] = cb[u];
      }
    }
#pragma unroll
    for (int u = 0; u < J; ++u) {
      const double diff = (double)xa[u] - (double)ca[u];
      s += diff * diff;
    }
    jj += J;
  }
  for (; jj < d; ++jj) {
    const double diff = (double)xr[jj] - (double)cr[jj];
    s += diff * diff;
  }
  return sqrt(s);
}

template <typename TC>
__global__ __launch_bounds__(256) void sp_nearest_candidates_kernel(const float* __restrict__ X, int64_t ldx,
                                                                    const TC* __restrict__ C, int64_t ldc, int kp,
                                                                    int k, int d, int64_t* __restrict__ labels,
                                                                    const int* __restrict__ rows,
                                                                    const int* __restrict__ n_rows, int64_t cap,
                                                                    const unsigned* __restrict__ cand_mask) {
  // A listed point has a handful of candidates (the centers inside its error window), and a candidate's distance is a
  // serial chain of d fused multiply-adds in cdist's order: a whole wave per point kept 2-8 of its 64 lanes busy.  GL
  // lanes take a point instead, 64 / GL points per wave (136 -> see profiles/r05_notes.md at configs[3]).
  constexpr int GL = 16, GROUPS = 64 / GL, LIST = 128;
  __shared__ int list_s[4][GROUPS][LIST];         // per group of lanes: the candidates of its point
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gl = lane & (GL - 1), grp = lane / GL;
  int* list = list_s[wv][grp];
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t count = *n_rows;
  if (count > cap) return;                        // no masks were written: the exact kernel re-does the list
  const int words = kp / 32;
  for (int64_t it0 = wave * GROUPS; it0 < count; it0 += nwaves * GROUPS) {
    const int64_t it = it0 + grp;
    const bool have = it < count;                 // (the groups of a wave walk together: shuffles and the wave barriers below)
    const int64_t row = have ? rows[it] : 0;
    const unsigned* __restrict__ mw = cand_mask + (have ? it : 0) * words;
    const float* __restrict__ xr = X + row * ldx;
    // ---- the list: word w of the mask holds centers 32 w .. 32 w + 31
    int total = 0;
    for (int w0 = 0; w0 < words; w0 += GL) {
      const int wi = w0 + gl;
      unsigned m = (have && wi < words) ? mw[wi] : 0u;
      if (wi * 32 + 32 > k) m &= wi * 32 < k ? ((1u << (k - wi * 32)) - 1u) : 0u;   // (padding centers)
      const int mine = __builtin_popcount(m);
      int inc = mine;
#pragma unroll
      for (int off = 1; off < GL; off <<= 1) {
        const int o = __shfl_up(inc, off, GL);
        if (gl >= off) inc += o;
      }
      int at = total + inc - mine;
      while (m) {
        if (at < LIST) list[at] = wi * 32 + __builtin_ctz(m);
        m &= m - 1;
        ++at;
      }
      total += __shfl(inc, GL - 1, GL);
    }
    __builtin_amdgcn_wave_barrier();
    int best_k = 0x7fffffff;
    double best = INFINITY;
    if (total == 1) {
      best_k = list[0];
    } else if (total > 1 && total <= LIST) {
      for (int c0 = 0; c0 < total; c0 += GL) {
        const bool live = c0 + gl < total;
        const int c = list[live ? c0 + gl : 0];
        const double s = km_exact_distance<TC>(xr, C + (int64_t)c * ldc, d);
        if (live && (s < best || (s == best && c < best_k))) {
          best = s;
          best_k = c;
        }
      }
    } else if (total > LIST) {
      // more candidates than the list holds (a mass of coincident centers): every lane walks the set bits of its
      // own words, one after the other
      for (int wi = gl; wi < words; wi += GL) {
        unsigned m = mw[wi];
        while (m) {
          const int c = wi * 32 + __builtin_ctz(m);
          m &= m - 1;
          if (c >= k) break;
          const double s = km_exact_distance<TC>(xr, C + (int64_t)c * ldc, d);
          if (s < best || (s == best && c < best_k)) {
            best = s;
            best_k = c;
          }
        }
      }
    }
    // (every group joins the shuffles: a group with one candidate or none brings its (best, best_k) as they are)
#pragma unroll
    for (int off = GL / 2; off > 0; off >>= 1) {
      const double ob = __shfl_xor(best, off, GL);
      const int ok = __shfl_xor(best_k, off, GL);
      if (total > 1 && (ob < best || (ob == best && ok < best_k))) {
        best = ob;
        best_k = ok;
      }
    }
    // (the window always contains the first pass's own best center; the guard is for NaN input)
    if (have && gl == 0) labels[row] = best_k == 0x7fffffff ? -1 - labels[row] : best_k;
    __builtin_amdgcn_wave_barrier();              // the list is rewritten for the next point
  }
}

// ------------------------------------------------------------------ bincount
__global__ __launch_bounds__(256) void sp_bincount_kernel(const int64_t* __restrict__ labels, int64_t n, int k,
                                                          unsigned long long* __restrict__ counts) {
  extern __shared__ int hist[];
  for (int i = threadIdx.x; i < k; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {      // four loads in flight per lane
    int64_t l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) l[u] = labels[i + u * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (l[u] >= 0 && l[u] < k) atomicAdd(&hist[(int)l[u]], 1);   // integer atomics: exact, order-free
  }
  for (; i < n; i += stride) {
    const int64_t l = labels[i];
    if (l >= 0 && l < k) atomicAdd(&hist[(int)l], 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += blockDim.x)
    if (hist[c]) atomicAdd(&counts[c], (unsigned long long)hist[c]);
}

// ------------------------------------------------------------------ stable counting sort of row ids by label
// hist[b][c] = number of rows of label c in row block b (row blocks of RB rows): rows of the table are written
// coalesced
__global__ __launch_bounds__(256) void sp_label_hist_kernel(const int64_t* __restrict__ labels, int64_t n, int k,
                                                            int rb, int nblk, int* __restrict__ hist) {
  extern __shared__ int lh[];
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < k; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)b * rb;
  const int64_t r1 = r0 + rb < n ? r0 + rb : n;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += blockDim.x) {
    const int64_t l = labels[i];
    if (l >= 0 && l < k) atomicAdd(&lh[(int)l], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += blockDim.x) hist[(int64_t)b * k + i] = lh[i];
}

// hist[b][c] <- number of rows of label c in the row blocks BEFORE b (exclusive scan down every column), and
// totals[c] = rows of label c.  One workgroup per 32 labels: 32 groups of threads walk 1/32 of the row blocks each
// (a wave reads two 128-B runs per step), the group sums are combined through LDS, and a second walk (the table is
// in L2 by then) writes the running counts.
constexpr int COLSCAN_LABELS = 32;
__global__ __launch_bounds__(1024) void sp_label_colscan_kernel(int* __restrict__ hist, int nblk, int k,
                                                                int* __restrict__ totals) {
  __shared__ int part[32][COLSCAN_LABELS + 1];
  const int ll = threadIdx.x & (COLSCAN_LABELS - 1), g = threadIdx.x / COLSCAN_LABELS;
  const int lab = blockIdx.x * COLSCAN_LABELS + ll;
  const int per = (nblk + 31) / 32;
  const int b0 = g * per < nblk ? g * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
  const int* __restrict__ col = hist + (lab < k ? lab : 0);
  int s = 0;
  if (lab < k) {
    int b = b0;
    for (; b + 8 <= b1; b += 8) {                    // eight loads in flight per lane
      int v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)(b + u) * k];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < b1; ++b) s += col[(int64_t)b * k];
  }
  part[g][ll] = s;
  __syncthreads();
  int pre = 0;
  for (int j = 0; j < g; ++j) pre += part[j][ll];
  if (lab < k) {
    if (g == 31) totals[lab] = pre + s;
    int* __restrict__ wcol = hist + lab;
    int run = pre;
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
      int v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = wcol[(int64_t)(b + u) * k];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        wcol[(int64_t)(b + u) * k] = run;
        run += v[u];
      }
    }
    for (; b < b1; ++b) {
      const int v = wcol[(int64_t)b * k];
      wcol[(int64_t)b * k] = run;
      run += v;
    }
  }
}

// perm[pos] = row, rows of one label contiguous and in ascending row order.
// One wavefront per row block; the LDS cursor of label c starts at (rows of the labels before c) + (rows of c in
// the row blocks before this one); every wave scans the k totals itself (64 B per lane), and the wave of block 0
// also writes seg_start[c] and slot_first[c] = first SEG_CHUNK-row chunk slot of label c.  Within a 64-row chunk a
// row's rank among the rows of its label is the number of LOWER lanes holding the same label (found with one
// ballot per label bit, no divergence); the last lane of each label advances the cursor (distinct addresses, no
// atomics).  The labels of RANK_AHEAD chunks are loaded before the first of them is ranked: the chain through the
// cursors is LDS-latency, not HBM-latency, bound.
constexpr int SEG_CHUNK = 512;
constexpr int RANK_AHEAD = 8;
__global__ __launch_bounds__(64) void sp_label_rank_kernel(const int64_t* __restrict__ labels, int64_t n, int k,
                                                           int rb, int nblk, const int* __restrict__ colpre,
                                                           const int* __restrict__ totals, int* __restrict__ perm,
                                                           int* __restrict__ seg_start, int* __restrict__ slot_first,
                                                           int64_t* __restrict__ counts) {
  extern __shared__ int cur[];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  int label_bits = 1;
  while ((1 << label_bits) < k) ++label_bits;
  {
    // label c = base + 64 u + lane: coalesced loads, eight in flight, one wave scan per 64 labels
    int carry = 0, carry2 = 0;
    const int* __restrict__ mine = colpre + (int64_t)b * k;
    for (int base = 0; base < k; base += 64 * 8) {
      int t[8], cp[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = base + u * 64 + lane;
        t[u] = c < k ? totals[c] : 0;
        cp[u] = c < k ? mine[c] : 0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = base + u * 64 + lane;
        if (base + u * 64 >= k) break;
        const int v = t[u], v2 = (t[u] + SEG_CHUNK - 1) / SEG_CHUNK;
        int inc = v, inc2 = v2;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_up(inc, off);
          if (lane >= off) inc += o;
        }
        if (b == 0) {
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const int o2 = __shfl_up(inc2, off);
            if (lane >= off) inc2 += o2;
          }
        }
        if (c < k) {
          cur[c] = carry + inc - v + cp[u];
          if (b == 0) {
            seg_start[c] = carry + inc - v;
            slot_first[c] = carry2 + inc2 - v2;
            if (counts) counts[c] = v;       // (np.bincount of the labels: the column totals of the histogram)
          }
        }
        carry += __shfl(inc, 63);
        if (b == 0) carry2 += __shfl(inc2, 63);
      }
    }
    if (b == 0 && lane == 0) {
      seg_start[k] = carry;
      slot_first[k] = carry2;
    }
  }
  __syncthreads();
  const int64_t r0 = (int64_t)b * rb;
  const int64_t r1 = r0 + rb < n ? r0 + rb : n;
  for (int64_t batch = r0; batch < r1; batch += 64 * RANK_AHEAD) {
    int64_t lraw[RANK_AHEAD];
#pragma unroll
    for (int u = 0; u < RANK_AHEAD; ++u) {
      const int64_t row = batch + u * 64 + lane;
      lraw[u] = row < r1 ? labels[row] : -1;
    }
#pragma unroll
    for (int u = 0; u < RANK_AHEAD; ++u) {
      const int64_t base = batch + u * 64;
      if (base >= r1) break;
      const int64_t row = base + lane;
      int lab = -1 - lane;                 // invalid rows: a value no other lane holds
      bool valid = false;
      if (lraw[u] >= 0 && lraw[u] < k) {
        lab = (int)lraw[u];
        valid = true;
      }
      // lanes holding the same label: the ballots of "my bit value", intersected bit by bit (label_bits <= 14
      // ballots instead of 64 readlane / compare steps)
      uint64_t peers = __ballot(valid);
      for (int bit = 0; bit < label_bits; ++bit) {
        const bool one = (lab >> bit) & 1;
        const uint64_t bal = __ballot(one);
        peers &= one ? bal : ~bal;
      }
      const int lower = __popcll(peers & ((1ull << lane) - 1ull));
      const int same = __popcll(peers);
      int start = 0;
      if (valid) start = cur[lab];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (LDS only: the perm stores of earlier chunks stay in flight)
      __builtin_amdgcn_wave_barrier();
      if (valid) {
        perm[start + lower] = (int)row;
        if (lower == same - 1) cur[lab] = start + same;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---- balanced, deterministic segment sums --------------------------------------------------
// The rows of a label are cut into chunks of SEG_CHUNK; chunk slots are numbered label-major (slot_first[c] = first
// chunk slot of label c, the exclusive scan of ceil(n_c / SEG_CHUNK) written by sp_label_rank_kernel).

// One wavefront per (chunk slot, 64*V-column block): the <= SEG_CHUNK rows of the chunk are added
// in ascending row order, one lane per V adjacent feature columns.  The row ids are fetched 64
// at a time with one coalesced load and broadcast from registers, so the row loads (64*V*sizeof(T)
// contiguous bytes each, U in flight) do not wait on an index load.  A label with at most
// SEG_CHUNK rows is therefore summed in exactly NumPy's axis-0 order.
template <typename T, int V>
__global__ __launch_bounds__(64) void sp_segment_sum_kernel(const T* __restrict__ X, int64_t ldx,
                                                            const int* __restrict__ perm,
                                                            const int* __restrict__ seg_start,
                                                            const int* __restrict__ slot_first, int k, int d,
                                                            T* __restrict__ partial) {
  constexpr int U = 8;
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int slot = blockIdx.x;
  if (slot >= slot_first[k]) return;
  // label of this slot: last c with slot_first[c] <= slot (binary search; empty labels own no slot)
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slot_first[mid] <= slot) lo = mid;
    else hi = mid - 1;
  }
  const int c = lo;
  const int lane = threadIdx.x;
  const int col = (blockIdx.y * 64 + lane) * V;
  const bool live = col < d;            // d % V == 0 (host-checked): a live lane owns V valid columns
  const int s0 = seg_start[c] + (slot - slot_first[c]) * SEG_CHUNK;
  const int s1 = s0 + SEG_CHUNK < seg_start[c + 1] ? s0 + SEG_CHUNK : seg_start[c + 1];
  T acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = (T)0;
  const T* __restrict__ Xc = X + (live ? col : 0);
  for (int base = s0; base < s1; base += 64) {
    const int cnt = s1 - base < 64 ? s1 - base : 64;
    const int pidx = lane < cnt ? perm[base + lane] : 0;
    int u0 = 0;
    for (; u0 + U <= cnt; u0 += U) {
      vec_t v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = __shfl(pidx, u0 + u);
        // every row is read exactly once: non-temporal (the tile is far bigger than the L2)
        if constexpr (V == 1) v[u][0] = __builtin_nontemporal_load(Xc + (int64_t)row * ldx);
        else v[u] = __builtin_nontemporal_load((const vec_t*)(Xc + (int64_t)row * ldx));
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += v[u][e];
    }
    for (; u0 < cnt; ++u0) {
      const int row = __shfl(pidx, u0);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += Xc[(int64_t)row * ldx + e];
    }
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < V; ++e) partial[(int64_t)slot * d + col + e] = acc[e];
  }
}

// out[c][col] = partial[first slot of c][col] + partial[next][col] + ... in slot order (0 for an empty label)
template <typename T>
__global__ __launch_bounds__(256) void sp_segment_combine_kernel(const T* __restrict__ partial,
                                                                 const int* __restrict__ slot_first, int k, int d,
                                                                 T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)k * d) return;
  const int c = (int)(i / d), col = (int)(i - (int64_t)c * d);
  const int f0 = slot_first[c], f1 = slot_first[c + 1];
  T acc = (T)0;
  if (f1 > f0) {
    // four slots' loads in flight; added in slot order
    T v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = f0 + u < f1 ? partial[(int64_t)(f0 + u) * d + col] : (T)0;
    acc = v[0];
#pragma unroll
    for (int u = 1; u < 4; ++u)
      if (f0 + u < f1) acc += v[u];
    for (int f = f0 + 4; f < f1; ++f) acc += partial[(int64_t)f * d + col];
  }
  out[i] = acc;
}

static int sort_block_rows(int64_t n, int64_t k) {
  // row-block size: keep the k x nblk histogram (scanned by one workgroup) under ~4M entries
  int64_t rb = 1024;
  while (((n + rb - 1) / rb) * k > (4LL << 20)) rb *= 2;
  return (int)rb;
}

}  // namespace

#include "kmeans_mfma.hpp"
#include "kmeans_split.hpp"

extern "C" size_t sp_nearest_center_workspace_bytes(int64_t n, int64_t k, int64_t d) {
  return sp_nearest_fused_ws_bytes(n, k, d);
}

// Which MFMA filter the AUTO / explicit tiers mean: the split tier wherever the fused one applies (fp32 points),
// unless the tier names the fp32 filter.
static bool km_use_split(int32_t tier, int64_t k, int64_t d, bool prepared) {
  if (tier == SP_NEAREST_SPLIT || tier == SP_NEAREST_SPLIT_UNCHECKED) return true;
  if (tier == SP_NEAREST_FUSED || tier == SP_NEAREST_FUSED_UNCHECKED) return false;
  // few features: the terms the split leaves out outweigh the roundings it saves.  A stand-alone call also pays for
  // cutting the points, which few centers do not earn back (tools/km_tier_sweep.py: 1 250 000 x 64, k = 64: 0.42 ms
  // fp32 / 0.50 split / 0.21 with prepared points; from k = 256 on the split wins either way)
  return d >= 32 && (prepared || k >= 192);
}

extern "C" size_t sp_kmeans_points_prepared_bytes(int64_t n, int64_t d) { return 256 + km_points_split_bytes(n, d); }

extern "C" int sp_kmeans_points_prepare(const float* d_points, int64_t ldx, int64_t n, int64_t d, void* d_prepared,
                                        size_t bytes, void* stream) {
  if (n < 0 || d < 0 || ldx < d) SP_FAIL("sp_kmeans_points_prepare: bad sizes");
  if (n == 0) return 0;
  if (!d_points || !d_prepared || bytes < sp_kmeans_points_prepared_bytes(n, d)) SP_FAIL("sp_kmeans_points_prepare: buffer too small");
  KmWorkspace w;
  w.dp = km_padded_features(d);
  km_carve_points((void*)(((uintptr_t)d_prepared + 255) & ~(uintptr_t)255), n, d, &w);
  // The shift: the mean of the points -- of every (n / 65536)-th of them when there are more than that.  Any vector is
  // a valid shift (kmeans_split.hpp: it moves the window's width, never a label); the mean of 65 thousand rows spread
  // over the tile is the mean of all of them to 0.4 % of a standard deviation, and reading 1.28 GB for it was a third
  // of a fit's set-up (220 + 113 us of 1.44 ms at configs[3]).
  const int64_t every = n > 2 * KM_MEAN_SAMPLE ? n / KM_MEAN_SAMPLE : 1;
  if (km_col_means<float>(d_points, ldx * every, n / every, d, w, (hipStream_t)stream)) return 1;
  return km_split_points(d_points, ldx, n, d, w, (hipStream_t)stream);
}

extern "C" size_t sp_nearest_center_prepared_workspace_bytes(int64_t n, int64_t k, int64_t d) {
  return sp_nearest_fused_ws_bytes(n, k, d, false);
}

static int km_nearest_center(const void* d_points, int32_t dtype, int64_t ldx, const void* d_prepared,
                             const void* d_centers, int32_t cdtype, int64_t ldc, int64_t n, int64_t k, int64_t d,
                             int64_t* d_labels, int32_t tier, void* d_ws, size_t ws_bytes, void* stream);

extern "C" int sp_nearest_center_prepared(const void* d_points, int32_t dtype, int64_t ldx, const void* d_prepared,
                                          const void* d_centers, int32_t cdtype, int64_t ldc, int64_t n, int64_t k,
                                          int64_t d, int64_t* d_labels, int32_t tier, void* d_ws, size_t ws_bytes,
                                          void* stream) {
  if (!d_prepared) SP_FAIL("sp_nearest_center_prepared: d_prepared is NULL");
  return km_nearest_center(d_points, dtype, ldx, d_prepared, d_centers, cdtype, ldc, n, k, d, d_labels, tier, d_ws,
                           ws_bytes, stream);
}

extern "C" int sp_nearest_center(const void* d_points, int32_t dtype, int64_t ldx, const void* d_centers,
                                 int32_t cdtype, int64_t ldc, int64_t n, int64_t k, int64_t d,
                                 int64_t* d_labels, int32_t tier, void* d_ws, size_t ws_bytes, void* stream) {
  return km_nearest_center(d_points, dtype, ldx, nullptr, d_centers, cdtype, ldc, n, k, d, d_labels, tier, d_ws, ws_bytes,
                           stream);
}

static int km_nearest_center(const void* d_points, int32_t dtype, int64_t ldx, const void* d_prepared,
                             const void* d_centers, int32_t cdtype, int64_t ldc, int64_t n, int64_t k, int64_t d,
                             int64_t* d_labels, int32_t tier, void* d_ws, size_t ws_bytes, void* stream) {
  if (n < 0 || k < 1 || d < 0) SP_FAIL("sp_nearest_center: bad sizes n=%lld k=%lld d=%lld", (long long)n, (long long)k, (long long)d);
  if (n == 0) return 0;
  if (!d_points || !d_centers || !d_labels) SP_FAIL("sp_nearest_center: NULL pointer");
  if ((dtype != SP_F32 && dtype != SP_F64) || (cdtype != SP_F32 && cdtype != SP_F64)) SP_FAIL("sp_nearest_center: points/centers must be f32 or f64");
  if (k > 2147483647LL || d > 2147483647LL) SP_FAIL("sp_nearest_center: k or d too large");
  if (ldx < d || ldc < d) SP_FAIL("sp_nearest_center: leading dimension too small");
  hipStream_t st = (hipStream_t)stream;
  const size_t need = sp_nearest_fused_ws_bytes(n, k, d, d_prepared == nullptr);
  if (!d_ws || ws_bytes < need) SP_FAIL("sp_nearest_center: workspace too small (%zu < %zu)", ws_bytes, need);
  KmWorkspace w = km_carve(d_ws, n, k, d);
  if (d_prepared) km_carve_points((void*)(((uintptr_t)d_prepared + 255) & ~(uintptr_t)255), n, d, &w);
  // fp64 transposed centers for the exact kernel
  {
    const int64_t tot = d * w.kp;
    const unsigned blocks = (unsigned)((tot + 255) / 256);
    if (tot > 0) {
      if (cdtype == SP_F32)
        hipLaunchKernelGGL((sp_centers_t64_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)d_centers, ldc,
                           (int)k, (int)d, (int)w.kp, w.Ct64);
      else
        hipLaunchKernelGGL((sp_centers_t64_kernel<double>), dim3(blocks), dim3(256), 0, st, (const double*)d_centers,
                           ldc, (int)k, (int)d, (int)w.kp, w.Ct64);
      SP_CHECK_LAUNCH();
    }
  }
  const int* rows = nullptr;
  const int* n_rows = nullptr;
  int64_t handled = -1;
  if (tier != SP_NEAREST_EXACT && dtype == SP_F32 && sp_nearest_fused_applicable(n, k, d, tier)) {
    const bool split = km_use_split(tier, k, d, d_prepared != nullptr);
    if (split) {
      if (!d_prepared) {      // the shift of a stand-alone call: the centers' mean (no extra pass over the points)
        if (cdtype == SP_F32 ? km_col_means<float>((const float*)d_centers, ldc, k, d, w, st)
                             : km_col_means<double>((const double*)d_centers, ldc, k, d, w, st)) return 1;
        if (km_split_points((const float*)d_points, ldx, n, d, w, st)) return 1;
      }
      if (sp_nearest_split_launch(d_centers, cdtype, ldc, n, k, d, d_labels, w, st)) return 1;
    } else {
      if (sp_nearest_fused_launch((const float*)d_points, ldx, d_centers, cdtype, ldc, n, k, d, d_labels, w, st)) return 1;
    }
    if (tier == SP_NEAREST_FUSED_UNCHECKED || tier == SP_NEAREST_SPLIT_UNCHECKED) return 0;   // diagnostics: leave the marks (-1 - best) in place
    // the points the fused kernel listed as undecided: the centers inside each one's window marked by the MFMA
    // filter, exact fp64 distances to those
    rows = w.amb_rows;
    n_rows = w.amb_count;
    if (split ? sp_nearest_split_mark_candidates(d, w, st) : sp_nearest_mark_candidates((const float*)d_points, ldx, d, w, st)) return 1;
    if (cdtype == SP_F32)
      hipLaunchKernelGGL((sp_nearest_candidates_kernel<float>), dim3(SP_CUS * 8), dim3(256), 0, st, (const float*)d_points,
                         ldx, (const float*)d_centers, ldc, (int)w.kp, (int)k, (int)d, d_labels, rows, n_rows, w.cand_cap,
                         w.cand_mask);
    else
      hipLaunchKernelGGL((sp_nearest_candidates_kernel<double>), dim3(SP_CUS * 8), dim3(256), 0, st, (const float*)d_points,
                         ldx, (const double*)d_centers, ldc, (int)w.kp, (int)k, (int)d, d_labels, rows, n_rows, w.cand_cap,
                         w.cand_mask);
    SP_CHECK_LAUNCH();
    handled = w.cand_cap;   // the exact kernel below only runs for a list the masks had no room for
  }
  const int64_t groups = (n + 7) / 8;   // 8 points per wave
  int64_t waves = rows ? (int64_t)SP_CUS * 16 : (groups < (int64_t)SP_CUS * 32 ? groups : (int64_t)SP_CUS * 32);
  const unsigned blocks = (unsigned)((waves + 3) / 4);
  if (dtype == SP_F32)
    hipLaunchKernelGGL((sp_nearest_exact_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)d_points, ldx,
                       w.Ct64, (int)w.kp, n, (int)k, (int)d, d_labels, rows, n_rows, handled);
  else
    hipLaunchKernelGGL((sp_nearest_exact_kernel<double>), dim3(blocks), dim3(256), 0, st, (const double*)d_points, ldx,
                       w.Ct64, (int)w.kp, n, (int)k, (int)d, d_labels, rows, n_rows, handled);
  SP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sp_bincount_i64(const int64_t* d_labels, int64_t n, int64_t k, int64_t* d_counts, void* stream) {
  if (n < 0 || k < 1) SP_FAIL("sp_bincount_i64: bad sizes");
  if (k > 16384) SP_FAIL("sp_bincount_i64: k=%lld exceeds the LDS histogram (16384)", (long long)k);
  if (!d_counts || (n && !d_labels)) SP_FAIL("sp_bincount_i64: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  SP_HIP(hipMemsetAsync(d_counts, 0, (size_t)k * 8, st));
  if (n == 0) return 0;
  // half the CUs, four loads in flight per lane: 8.9 us on 1.25 M labels / 1024 bins against 13.2 us for 1024
  // workgroups (each workgroup ends with up to k global atomics)
  int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);
  if (blocks > SP_CUS / 2) blocks = SP_CUS / 2;
  hipLaunchKernelGGL(sp_bincount_kernel, dim3((unsigned)blocks), dim3(256), (size_t)k * 4, st, d_labels, n, (int)k,
                     (unsigned long long*)d_counts);
  SP_CHECK_LAUNCH();
  return 0;
}

static int64_t seg_max_slots(int64_t n, int64_t k) { return k + n / SEG_CHUNK; }

static size_t seg_int_words(int64_t n, int64_t k) {
  const int64_t rb = sort_block_rows(n, k);
  const int64_t nblk = (n + rb - 1) / rb;
  return (size_t)(k * nblk + n + (k + 1) + k + (k + 1));
}

extern "C" size_t sp_segment_sum_workspace_bytes(int64_t n, int64_t k, int64_t d) {
  if (n < 1 || k < 1) return 256;
  return ((seg_int_words(n, k) * 4 + 255) & ~(size_t)255) + (size_t)seg_max_slots(n, k) * (size_t)(d < 1 ? 1 : d) * 8 + 512;
}

extern "C" int sp_segment_sum(const void* d_points, int32_t dtype, int64_t ldx, const int64_t* d_labels, int64_t n,
                              int64_t k, int64_t d, void* d_out, void* d_ws, size_t ws_bytes, void* stream) {
  return sp_segment_sum_counts(d_points, dtype, ldx, d_labels, n, k, d, d_out, nullptr, d_ws, ws_bytes, stream);
}

extern "C" int sp_segment_sum_counts(const void* d_points, int32_t dtype, int64_t ldx, const int64_t* d_labels, int64_t n,
                                     int64_t k, int64_t d, void* d_out, int64_t* d_counts, void* d_ws, size_t ws_bytes,
                                     void* stream) {
  if (n < 0 || k < 1 || d < 0) SP_FAIL("sp_segment_sum: bad sizes");
  if (dtype != SP_F32 && dtype != SP_F64) SP_FAIL("sp_segment_sum: points must be f32 or f64");
  if (k > 16384) SP_FAIL("sp_segment_sum: k=%lld exceeds the LDS cursor table (16384)", (long long)k);
  if (n > 2147483647LL || d > 2147483647LL) SP_FAIL("sp_segment_sum: n or d too large");
  if (!d_out || (n && (!d_points || !d_labels))) SP_FAIL("sp_segment_sum: NULL pointer");
  if (ldx < d) SP_FAIL("sp_segment_sum: leading dimension too small");
  hipStream_t st = (hipStream_t)stream;
  const size_t esz = dtype == SP_F32 ? 4 : 8;
  if (n == 0 || d == 0) {
    SP_HIP(hipMemsetAsync(d_out, 0, (size_t)k * (size_t)d * esz, st));
    return d_counts ? sp_bincount_i64(d_labels, n, k, d_counts, stream) : 0;
  }
  if (!d_ws || ws_bytes < sp_segment_sum_workspace_bytes(n, k, d)) SP_FAIL("sp_segment_sum: workspace too small");
  const int rb = sort_block_rows(n, k);
  const int nblk = (int)((n + rb - 1) / rb);
  int* hist = (int*)d_ws;                    // [nblk][k]
  int* perm = hist + (int64_t)k * nblk;      // [n]
  int* seg = perm + n;                       // [k + 1]
  int* totals = seg + k + 1;                 // [k]
  int* slot_first = totals + k;              // [k + 1]
  void* partial = (char*)d_ws + ((seg_int_words(n, k) * 4 + 255) & ~(size_t)255);   // [max slots][d]
  hipLaunchKernelGGL(sp_label_hist_kernel, dim3(nblk), dim3(256), (size_t)k * 4, st, d_labels, n, (int)k, rb, nblk, hist);
  SP_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_label_colscan_kernel, dim3((unsigned)((k + COLSCAN_LABELS - 1) / COLSCAN_LABELS)), dim3(1024), 0, st,
                     hist, nblk, (int)k, totals);
  SP_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_label_rank_kernel, dim3(nblk), dim3(64), (size_t)k * 4, st, d_labels, n, (int)k, rb, nblk,
                     hist, totals, perm, seg, slot_first, d_counts);
  SP_CHECK_LAUNCH();
  const int64_t max_slots = seg_max_slots(n, k);
  // V columns per lane: as wide as alignment allows while the launch still has >= 2048 waves
  const size_t vbytes = esz;
  int V = 1;
  for (int cand = 4; cand > 1; cand >>= 1) {
    const bool aligned = (d % cand == 0) && (ldx % cand == 0) && ((((uintptr_t)d_points) % (cand * vbytes)) == 0);
    if (aligned && max_slots * ((d + 64 * cand - 1) / (64 * cand)) >= 2048) {
      V = cand;
      break;
    }
  }
  const dim3 grid((unsigned)max_slots, (unsigned)((d + 64 * V - 1) / (64 * V)));
#define SP_SEG_GO(T, VV)                                                                                      \
  hipLaunchKernelGGL((sp_segment_sum_kernel<T, VV>), grid, dim3(64), 0, st, (const T*)d_points, ldx, perm, seg, \
                     slot_first, (int)k, (int)d, (T*)partial)
  if (dtype == SP_F32) {
    if (V == 4) SP_SEG_GO(float, 4);
    else if (V == 2) SP_SEG_GO(float, 2);
    else SP_SEG_GO(float, 1);
  } else {
    if (V == 4) SP_SEG_GO(double, 4);
    else if (V == 2) SP_SEG_GO(double, 2);
    else SP_SEG_GO(double, 1);
  }
#undef SP_SEG_GO
  SP_CHECK_LAUNCH();
  const unsigned cblocks = (unsigned)((k * d + 255) / 256);
  if (dtype == SP_F32)
    hipLaunchKernelGGL((sp_segment_combine_kernel<float>), dim3(cblocks), dim3(256), 0, st, (const float*)partial,
                       slot_first, (int)k, (int)d, (float*)d_out);
  else
    hipLaunchKernelGGL((sp_segment_combine_kernel<double>), dim3(cblocks), dim3(256), 0, st, (const double*)partial,
                       slot_first, (int)k, (int)d, (double*)d_out);
  SP_CHECK_LAUNCH();
  return 0;
}
