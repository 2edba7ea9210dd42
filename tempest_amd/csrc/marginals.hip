// Posterior marginals on the device (tph_marginals; DESIGN.md section 13a, KERNELS.md 3u): weighted mean, variance, range,
// 1-D and 2-D histograms and quantiles of every column of m ROW-MAJOR rows v (m, c), c <= 128, with weights w (m).
//
// W = sum w, u_i = w_i / W (one division), k_i = llrint(u_i 2^52).  Every floating-point sum over rows runs in ONE order --
// chunks of MG_CHUNK = 64 consecutive rows added by tph_wave_sum's shuffle tree, blocks of MG_BLOCK = 16 chunk sums in chunk order,
// the block sums in block order, every level from +0.0, the last chunk / block simply shorter -- and every table is a sum of the
// 64-bit integers k_i, so no tile, slab, batch or atomic order changes a bit of any output.  No floating-point atomics.
//
// How the rows reach the lanes: a workgroup takes 256 rows x a tile of `ct` columns through LDS -- the ct-long runs of every row
// are read by consecutive lanes (whole sectors from ct = 8 on, the whole contiguous block where ct = c), stored at a pitch of
// tile | 1 doubles, and lane t then reads row t column by column without a bank conflict.  The same form at every c up to 128.
#include <string.h>
#include <algorithm>

#include "common.h"

// every product and sum below is rounded once: what a NumPy restatement computes
#pragma clang fp contract(off)

constexpr int MG_CHUNK = 64, MG_BLOCK = 16;
constexpr int64_t MG_SPAN = (int64_t)MG_CHUNK * MG_BLOCK;
constexpr int MG_MAX_C = 128, MG_MAX_BINS = 1024, MG_MAX_BINS2 = 128, MG_MAX_Q = 8;
constexpr int MG_SWEEP_CT = 16;            // columns per workgroup of the moment sweeps, at most: 256 x 17 x 8 B of rows
constexpr int MG_HIST_CT = 8;              // columns per workgroup of the 1-D histogram and the select, at most
constexpr int MG_HIST_WORDS = 4100;        // 8-byte cells of 1-D tables a workgroup holds: 4 columns of 1024 bins + outside
constexpr int MG_SEL_TAB = 16;             // (column, q) bucket tables of 256 x 8 B a workgroup of the select holds: 32 KiB
constexpr int MG_LDS2 = 64;                // bins_2d up to which the 2-D table sits in LDS (64 x 64 x 8 B = 32 KiB)
constexpr int MG_PASSES = 8;
constexpr int64_t MG_BATCH_WORDS = (int64_t)1 << 23;
constexpr int MG_MIN_WG = 1024;            // workgroups a grid is cut for (4 per CU of a 256-CU device)
static_assert(MG_CHUNK == TPH_WAVE, "a chunk of rows is a wave");
static_assert(TPH_MARGINALS_TILES == 7, "tiles_host layout");

struct mg_qs { double q[MG_MAX_Q]; };

__device__ __forceinline__ double mg_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned long long mg_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// the integer weight of a row
__device__ __forceinline__ unsigned long long mg_k(double wi, double W) {
  const double u = wi > 0.0 ? wi / W : 0.0;
  return (unsigned long long)llrint(u * 4503599627370496.0);
}
// bin of v among B bins of [lo, hi] (inv = B / (hi - lo), from the host), or -1: outside, NaN, +-inf
__device__ __forceinline__ int mg_bin(double v, double lo, double hi, double inv, int B) {
  if (!(v >= lo && v <= hi)) return -1;
  if (v == hi) return B - 1;
  const double d = v - lo;
  const double t = d * inv;
  if (!(t < (double)B)) return B - 1;
  return (int)(long long)t;
}
// order-preserving key of a double (no NaN comes here): negative values all bits flipped, the others the sign bit
__device__ __forceinline__ unsigned long long mg_key(double p) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(p);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// rows row0 .. row0 + rows - 1 (rows <= 256), columns j0 .. j0 + ct - 1 of x (n, c) into s_x[row * pitch + column - j0]
__device__ __forceinline__ void mg_stage(const double* __restrict__ x, int64_t row0, int rows, int c, int j0, int ct, int pitch,
                                         double* __restrict__ s_x) {
  __syncthreads();                   // (the previous tile has been taken out of s_x)
  const int cnt = rows * ct;
  for (int e = threadIdx.x; e < cnt; e += 256) {
    const int r = e / ct, jj = e - r * ct;
    s_x[r * pitch + jj] = x[(size_t)(row0 + r) * (size_t)c + (size_t)(j0 + jj)];
  }
  __syncthreads();
}

// ---- W = sum w: block sums, then the fold ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mg_wsum(const double* __restrict__ w, int64_t n, double* __restrict__ wpart) {
  __shared__ double s_c[MG_BLOCK];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * MG_SPAN, b1 = b0 + MG_SPAN < n ? b0 + MG_SPAN : n;
  const int nch = (int)((b1 - b0 + MG_CHUNK - 1) / MG_CHUNK);
  for (int64_t row0 = b0; row0 < b1; row0 += 256) {
    const int64_t i = row0 + threadIdx.x;
    const double v = tph_wave_sum(i < b1 ? w[i] : 0.0);
    const int ch = (int)((row0 - b0) / MG_CHUNK) + wid;
    if (lane == 0 && ch < nch) s_c[ch] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double bs = 0.0;
    for (int ch = 0; ch < nch; ++ch) bs += s_c[ch];
    wpart[blockIdx.x] = bs;
  }
}
__global__ void k_mg_wfold(const double* __restrict__ wpart, int64_t nblocks, double* __restrict__ W) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double tot = 0.0;
  for (int64_t b = 0; b < nblocks; ++b) tot += wpart[b];
  W[0] = tot;
}
// sum of the integer weights
__global__ void __launch_bounds__(256) k_mg_sumk(const double* __restrict__ w, int64_t n, const double* __restrict__ Wp,
                                                 unsigned long long* __restrict__ sumk) {
  const double W = Wp[0];
  unsigned long long acc = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += mg_k(w[i], W);
  acc = mg_wave_sum_u64(acc);
  if ((threadIdx.x & 63) == 0 && acc != 0ull) atomicAdd(sumk, acc);
}

// ---- moment sweeps ----------------------------------------------------------------------------------------------------------------
// MODE 0: block sums of u_i v_ij and, with want_range, the block's min / max over the finite v_ij of rows with w_i > 0; MODE 1: block
// sums of u_i (v_ij - mean_j)^2.  Columns j_lo .. j_hi - 1 (a batch), `tile` of them per workgroup (grid y), one block of MG_SPAN rows
// per workgroup (grid x); part / pmin / pmax [row block][j - j_lo], mean indexed by the column itself.
template <int MODE>
__global__ void __launch_bounds__(256) k_mg_sweep(const double* __restrict__ x, const double* __restrict__ w, int64_t n, int c,
                                                  const double* __restrict__ Wp, int j_lo, int j_hi, int tile, int want_range,
                                                  const double* __restrict__ mean, double* __restrict__ part,
                                                  double* __restrict__ pmin, double* __restrict__ pmax) {
  __shared__ double s_x[256 * (MG_SWEEP_CT | 1)];
  __shared__ double s_cs[MG_SWEEP_CT * MG_BLOCK];
  __shared__ double s_mn[MODE == 0 ? MG_SWEEP_CT * MG_BLOCK : 1], s_mx[MODE == 0 ? MG_SWEEP_CT * MG_BLOCK : 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j0 = j_lo + (int)blockIdx.y * tile, j1 = j0 + tile < j_hi ? j0 + tile : j_hi, ct = j1 - j0, nb = j_hi - j_lo;
  const int pitch = tile | 1;
  const int64_t b0 = (int64_t)blockIdx.x * MG_SPAN, b1 = b0 + MG_SPAN < n ? b0 + MG_SPAN : n;
  const int nch = (int)((b1 - b0 + MG_CHUNK - 1) / MG_CHUNK);
  const double W = Wp[0];
  for (int64_t row0 = b0; row0 < b1; row0 += 256) {
    const int rows = (int)(b1 - row0 < 256 ? b1 - row0 : 256);
    mg_stage(x, row0, rows, c, j0, ct, pitch, s_x);
    const bool has = (int)threadIdx.x < rows;
    double u = 0.0;
    bool wpos = false;
    if (has) {
      const double wi = w[row0 + threadIdx.x];
      wpos = wi > 0.0;
      u = wpos ? wi / W : 0.0;
    }
    const int ch = (int)((row0 - b0) / MG_CHUNK) + wid;
    for (int jj = 0; jj < ct; ++jj) {
      const double v = has ? s_x[threadIdx.x * pitch + jj] : 0.0;
      double t;
      if (MODE == 0) {
        t = u * v;
      } else {
        const double d = v - mean[j0 + jj];
        const double d2 = d * d;
        t = u * d2;
      }
      t = tph_wave_sum(u > 0.0 ? t : 0.0);       // (a row without weight adds +0.0 whatever v holds)
      if (lane == 0 && ch < nch) s_cs[jj * MG_BLOCK + ch] = t;
      if (MODE == 0 && want_range) {
        const bool fin = wpos && fabs(v) <= DBL_MAX;
        const double mn = mg_wave_min(fin ? v : INFINITY), mx = tph_wave_max(fin ? v : -INFINITY);
        if (lane == 0 && ch < nch) { s_mn[jj * MG_BLOCK + ch] = mn; s_mx[jj * MG_BLOCK + ch] = mx; }
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < ct; t += 256) {
    double bs = 0.0;
    for (int ch = 0; ch < nch; ++ch) bs += s_cs[t * MG_BLOCK + ch];
    const size_t o = (size_t)blockIdx.x * (size_t)nb + (size_t)(j0 - j_lo + t);
    part[o] = bs;
    if (MODE == 0 && want_range) {
      double mn = INFINITY, mx = -INFINITY;
      for (int ch = 0; ch < nch; ++ch) { mn = fmin(mn, s_mn[t * MG_BLOCK + ch]); mx = fmax(mx, s_mx[t * MG_BLOCK + ch]); }
      pmin[o] = mn;
      pmax[o] = mx;
    }
  }
}
// out[j] = the block sums of column j in block order
__global__ void __launch_bounds__(256) k_mg_fold(const double* __restrict__ part, int64_t nblocks, int nb, double* __restrict__ out) {
  const int r = (int)blockIdx.x * 256 + threadIdx.x;
  if (r >= nb) return;
  double tot = 0.0;
  for (int64_t b = 0; b < nblocks; ++b) tot += part[(size_t)b * (size_t)nb + r];
  out[r] = tot;
}
// range[j] = (min, max) over the blocks: (+inf, -inf) where no row of the column has weight and a finite value
__global__ void __launch_bounds__(256) k_mg_fold_range(const double* __restrict__ pmin, const double* __restrict__ pmax, int64_t nblocks,
                                                       int nb, double* __restrict__ range) {
  const int r = (int)blockIdx.x * 256 + threadIdx.x;
  if (r >= nb) return;
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t b = 0; b < nblocks; ++b) {
    mn = fmin(mn, pmin[(size_t)b * (size_t)nb + r]);
    mx = fmax(mx, pmax[(size_t)b * (size_t)nb + r]);
  }
  range[2 * r] = mn;
  range[2 * r + 1] = mx;
}

// ---- 1-D histograms -----------------------------------------------------------------------------------------------------------------
// A workgroup takes `slab` rows (grid x; a multiple of 256) and `tile` columns (grid y; tile * (B + 1) <= MG_HIST_WORDS), keeps their
// tables -- B bins and the outside cell each -- in LDS and adds what is not zero to counts [c][B] / outside [c] at the end.
// par = lo[128], hi[128], inv[128] (, inv of the 2-D tables [128]).
__global__ void __launch_bounds__(256) k_mg_hist1(const double* __restrict__ x, const double* __restrict__ w, int64_t n, int c,
                                                  const double* __restrict__ Wp, const double* __restrict__ par, int B, int tile,
                                                  int64_t slab, unsigned long long* __restrict__ counts,
                                                  unsigned long long* __restrict__ outside) {
  __shared__ double s_x[256 * (MG_HIST_CT | 1)];
  __shared__ unsigned long long s_tab[MG_HIST_WORDS];
  const int j0 = (int)blockIdx.y * tile, ct = j0 + tile < c ? tile : c - j0, pitch = tile | 1, B1 = B + 1;
  const int64_t b0 = (int64_t)blockIdx.x * slab, b1 = b0 + slab < n ? b0 + slab : n;
  const int cells = ct * B1;
  for (int e = threadIdx.x; e < cells; e += 256) s_tab[e] = 0ull;
  const double W = Wp[0];
  for (int64_t row0 = b0; row0 < b1; row0 += 256) {
    const int rows = (int)(b1 - row0 < 256 ? b1 - row0 : 256);
    mg_stage(x, row0, rows, c, j0, ct, pitch, s_x);
    if ((int)threadIdx.x < rows) {
      const unsigned long long k = mg_k(w[row0 + threadIdx.x], W);
      if (k != 0ull) {
        for (int jj = 0; jj < ct; ++jj) {
          const int j = j0 + jj;
          const int b = mg_bin(s_x[threadIdx.x * pitch + jj], par[j], par[MG_MAX_C + j], par[2 * MG_MAX_C + j], B);
          atomicAdd(&s_tab[jj * B1 + (b < 0 ? B : b)], k);
        }
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cells; e += 256) {
    const unsigned long long v = s_tab[e];
    if (v != 0ull) {
      const int jj = e / B1, b = e - jj * B1;
      if (b == B) atomicAdd(outside + j0 + jj, v);
      else atomicAdd(counts + (size_t)(j0 + jj) * (size_t)B + (size_t)b, v);
    }
  }
}

// ---- 2-D histograms -----------------------------------------------------------------------------------------------------------------
// Grid (rows of `slab`, pair).  The two values of a row are read where they lie: the workgroups of one slab -- every pair of it --
// run side by side and find the rows in L2.  LDS: the B2 x B2 table (B2 <= MG_LDS2) in LDS, flushed like the 1-D one; otherwise
// every row adds straight to the table in memory.  A row with either value outside goes to outside2[pair], summed per wave first.
template <bool LDS>
__global__ void __launch_bounds__(256) k_mg_hist2(const double* __restrict__ x, const double* __restrict__ w, int64_t n, int c,
                                                  const double* __restrict__ Wp, const double* __restrict__ par,
                                                  const int32_t* __restrict__ pairs, int B2, int64_t slab,
                                                  unsigned long long* __restrict__ counts2, unsigned long long* __restrict__ outside2) {
  __shared__ unsigned long long s_tab[LDS ? MG_LDS2 * MG_LDS2 : 1];
  const int p = (int)blockIdx.y, a = pairs[2 * p], b = pairs[2 * p + 1];
  const double lo_a = par[a], hi_a = par[MG_MAX_C + a], inv_a = par[3 * MG_MAX_C + a];
  const double lo_b = par[b], hi_b = par[MG_MAX_C + b], inv_b = par[3 * MG_MAX_C + b];
  const int64_t b0 = (int64_t)blockIdx.x * slab, b1 = b0 + slab < n ? b0 + slab : n;
  const int cells = B2 * B2;
  unsigned long long* dst = counts2 + (size_t)p * (size_t)cells;
  if (LDS) {
    for (int e = threadIdx.x; e < cells; e += 256) s_tab[e] = 0ull;
    __syncthreads();
  }
  const double W = Wp[0];
  unsigned long long out = 0ull;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) {
    const unsigned long long k = mg_k(w[i], W);
    if (k != 0ull) {
      const int ba = mg_bin(x[(size_t)i * (size_t)c + (size_t)a], lo_a, hi_a, inv_a, B2);
      const int bb = mg_bin(x[(size_t)i * (size_t)c + (size_t)b], lo_b, hi_b, inv_b, B2);
      if (ba < 0 || bb < 0) out += k;
      else atomicAdd((LDS ? s_tab : dst) + ba * B2 + bb, k);
    }
  }
  out = mg_wave_sum_u64(out);
  if ((threadIdx.x & 63) == 0 && out != 0ull) atomicAdd(outside2 + p, out);
  if (LDS) {
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += 256) {
      const unsigned long long v = s_tab[e];
      if (v != 0ull) atomicAdd(dst + e, v);
    }
  }
}

// ---- quantiles: radix select on the order-preserving key, 8 passes of 8 bits ---------------------------------------------------
// One pass: every row adds k to bucket (key >> shift) & 255 of each (column, q) whose prefix its key carries (pass 0: all of them).  A
// workgroup takes `slab` rows (grid x) and `tile` columns of the batch j_lo .. j_hi - 1 (grid y; tile * nq <= MG_SEL_TAB), keeps
// their tables in LDS and adds what is not zero to hist [j - j_lo][q][256].  nanflag[j - j_lo] != 0: a NaN with k > 0 (pass 0 looks).
__global__ void __launch_bounds__(256) k_mg_sel_hist(const double* __restrict__ x, const double* __restrict__ w, int64_t n, int c,
                                                     const double* __restrict__ Wp, int j_lo, int j_hi, int tile, int64_t slab, int nq,
                                                     int pass, const unsigned long long* __restrict__ prefix,
                                                     unsigned long long* __restrict__ hist, unsigned long long* __restrict__ nanflag) {
  __shared__ double s_x[256 * (MG_HIST_CT | 1)];
  __shared__ unsigned long long s_tab[MG_SEL_TAB * 256];
  const int lane = threadIdx.x & 63;
  const int j0 = j_lo + (int)blockIdx.y * tile, j1 = j0 + tile < j_hi ? j0 + tile : j_hi, ct = j1 - j0, pitch = tile | 1;
  const int64_t b0 = (int64_t)blockIdx.x * slab, b1 = b0 + slab < n ? b0 + slab : n;
  const int cells = ct * nq * 256;
  for (int e = threadIdx.x; e < cells; e += 256) s_tab[e] = 0ull;
  const double W = Wp[0];
  const int shift = 56 - 8 * pass;
  for (int64_t row0 = b0; row0 < b1; row0 += 256) {
    const int rows = (int)(b1 - row0 < 256 ? b1 - row0 : 256);
    mg_stage(x, row0, rows, c, j0, ct, pitch, s_x);
    const bool has = (int)threadIdx.x < rows;
    const unsigned long long k = has ? mg_k(w[row0 + threadIdx.x], W) : 0ull;
    for (int jj = 0; jj < ct; ++jj) {
      const double v = has ? s_x[threadIdx.x * pitch + jj] : 0.0;
      const bool isn = v != v;
      if (pass == 0 && __ballot(isn && k != 0ull) != 0ull && lane == 0) atomicOr(&nanflag[j0 - j_lo + jj], 1ull);
      if (k != 0ull && !isn) {
        const unsigned long long key = mg_key(v);
        const int digit = (int)((key >> shift) & 255ull);
        unsigned long long* tab = s_tab + (size_t)jj * nq * 256 + digit;
        const unsigned long long head = pass == 0 ? 0ull : key >> (shift + 8);
        for (int q = 0; q < nq; ++q)
          if (pass == 0 || head == prefix[(j0 - j_lo + jj) * nq + q]) atomicAdd(tab + q * 256, k);
      }
    }
  }
  __syncthreads();
  unsigned long long* dst = hist + (size_t)(j0 - j_lo) * nq * 256;
  for (int e = threadIdx.x; e < cells; e += 256) {
    const unsigned long long v = s_tab[e];
    if (v != 0ull) atomicAdd(dst + e, v);
  }
}
// A wave per (column, q): the first bucket at which the running total reaches the target becomes the next 8 bits of the prefix, the
// target what is left inside that bucket; the buckets are zeroed for the next pass.  Pass 0 sets the target: ceil(q 2^52) held
// inside [1, total].  The last pass turns the key back into the double: quant[q][j_lo + column].
__global__ void __launch_bounds__(256) k_mg_sel_narrow(unsigned long long* __restrict__ hist, unsigned long long* __restrict__ prefix,
                                                       unsigned long long* __restrict__ target,
                                                       const unsigned long long* __restrict__ nanflag, int nb, int nq, int pass, mg_qs qs,
                                                       double* __restrict__ quant, int j_lo, int c) {
  const int lane = threadIdx.x & 63;
  const int g = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nb * nq) return;
  unsigned long long* h = hist + (size_t)g * 256 + 4 * lane;
  unsigned long long a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { a[j] = h[j]; h[j] = 0ull; }
  const unsigned long long own = (a[0] + a[1]) + (a[2] + a[3]);
  unsigned long long s = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  const unsigned long long total = __shfl(s, 63, 64);
  const int rl = g / nq, q = g % nq;
  const bool last = pass == MG_PASSES - 1;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (total == 0ull) {               // no row with weight and a number: NaN
    if (lane == 0) { prefix[g] = 0ull; target[g] = 0ull; if (last) quant[(size_t)q * c + j_lo + rl] = nan; }
    return;
  }
  unsigned long long T;
  if (pass == 0) {
    T = (unsigned long long)ceil(qs.q[q] * 4503599627370496.0);
    T = T < 1ull ? 1ull : (T > total ? total : T);
  } else {
    T = target[g];
  }
  const unsigned long long reach = __ballot(s >= T);
  const int first = __ffsll((long long)reach) - 1;
  if (lane == first) {
    unsigned long long cum = s - own;
    const unsigned long long c0 = cum + a[0], c1 = c0 + a[1], c2 = c1 + a[2];
    int j = 0;
    if (c0 < T) { j = 1; cum = c0; }
    if (c1 < T) { j = 2; cum = c1; }
    if (c2 < T) { j = 3; cum = c2; }
    const unsigned long long pre = ((pass == 0 ? 0ull : prefix[g]) << 8) | (unsigned long long)(4 * lane + j);
    prefix[g] = pre;
    target[g] = T - cum;
    if (last) {
      const unsigned long long bits = (pre >> 63) ? (pre & 0x7fffffffffffffffull) : ~pre;
      quant[(size_t)q * c + j_lo + rl] = nanflag[rl] ? nan : __longlong_as_double((long long)bits);
    }
  }
}
#pragma clang fp contract(on)

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static inline int64_t mg_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t mg_fixed_words(int64_t nblocks, int n_pairs) { return 1 + nblocks + 4 * MG_MAX_C + n_pairs; }
static inline int64_t mg_col_words(int64_t nblocks, int n_q) { return 3 * nblocks + 258 * (int64_t)n_q + 1; }
static inline int mg_batch_cols(int64_t nblocks, int c, int n_q, int64_t cap) {
  const int64_t fit = cap / mg_col_words(nblocks, n_q);
  return (int)(fit < 1 ? 1 : (fit > c ? c : fit));
}
// rows per workgroup (a multiple of 256) that bring a grid of `tiles_y` column tiles / pairs to MG_MIN_WG workgroups
static inline int64_t mg_slab(int64_t m, int64_t tiles_y) {
  const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(mg_ceil_div(m, 256), mg_ceil_div(MG_MIN_WG, tiles_y)));
  return std::max<int64_t>(256, mg_ceil_div(mg_ceil_div(m, slabs), 256) * 256);
}

extern "C" int64_t tph_marginals_layout(int which) {
  switch (which) {
    case 0: return MG_CHUNK;
    case 1: return MG_BLOCK;
    case 2: return MG_MAX_C;
    case 3: return MG_MAX_BINS;
    case 4: return MG_MAX_BINS2;
    case 5: return MG_MAX_Q;
    case 6: return MG_BATCH_WORDS;
    case 7: return TPH_MARGINALS_TILES;
    default: return -1;
  }
}

extern "C" int64_t tph_marginals_scratch_words(int64_t m, int c, int bins, int n_pairs, int bins_2d, int n_q) {
  if (m < 1 || c < 1 || c > MG_MAX_C || bins < 1 || bins > MG_MAX_BINS || n_pairs < 0 || n_q < 0 || n_q > MG_MAX_Q ||
      (n_pairs > 0 && (bins_2d < 1 || bins_2d > MG_MAX_BINS2)))
    return -1;
  const int64_t nblocks = mg_ceil_div(m, MG_SPAN);
  return mg_fixed_words(nblocks, n_pairs) + mg_col_words(nblocks, n_q) * mg_batch_cols(nblocks, c, n_q, MG_BATCH_WORDS);
}

extern "C" int tph_marginals(tph_ctx* ctx, const double* rows_dev, int64_t m, int c, const double* w_dev, const double* range_host,
                             int bins, const int32_t* pairs_host, int n_pairs, int bins_2d, const double* q_host, int n_q,
                             const int32_t* tiles_host, int64_t* scratch_dev, int64_t scratch_words, double* moments_dev,
                             double* range_dev, double* quant_dev, int64_t* counts_dev, int64_t* outside_dev, int64_t* counts2d_dev,
                             int64_t* outside2d_dev, int64_t* sumk_dev) {
  TPH_REQUIRE(ctx && rows_dev && w_dev && scratch_dev && moments_dev && range_dev && counts_dev && outside_dev && sumk_dev,
              "tph_marginals: NULL argument");
  TPH_REQUIRE(m >= 1 && c >= 1 && c <= MG_MAX_C, "tph_marginals: need m >= 1 and 1 <= c <= %d (m = %lld, c = %d)", MG_MAX_C, (long long)m, c);
  TPH_REQUIRE(bins >= 1 && bins <= MG_MAX_BINS, "tph_marginals: bins must be 1 .. %d, got %d", MG_MAX_BINS, bins);
  TPH_REQUIRE(n_q >= 0 && n_q <= MG_MAX_Q && (n_q == 0 || (q_host && quant_dev)), "tph_marginals: at most %d quantiles, with their arrays", MG_MAX_Q);
  TPH_REQUIRE(n_pairs >= 0 && n_pairs <= 65535, "tph_marginals: bad n_pairs %d", n_pairs);
  TPH_REQUIRE(n_pairs == 0 || (pairs_host && counts2d_dev && outside2d_dev && bins_2d >= 1 && bins_2d <= MG_MAX_BINS2),
              "tph_marginals: pairs need their arrays and bins_2d of 1 .. %d, got %d", MG_MAX_BINS2, bins_2d);
  mg_qs qs{};
  for (int q = 0; q < n_q; ++q) {
    TPH_REQUIRE(q_host[q] >= 0.0 && q_host[q] <= 1.0, "tph_marginals: quantile %d is not in [0, 1]", q);
    qs.q[q] = q_host[q];
  }
  for (int p = 0; p < n_pairs; ++p) {
    const int a = pairs_host[2 * p], b = pairs_host[2 * p + 1];
    TPH_REQUIRE(a >= 0 && a < c && b >= 0 && b < c && a != b, "tph_marginals: pair %d = (%d, %d) is not two different columns below %d", p, a, b, c);
  }
  if (range_host)
    for (int j = 0; j < c; ++j)
      TPH_REQUIRE(fabs(range_host[2 * j]) <= DBL_MAX && fabs(range_host[2 * j + 1]) <= DBL_MAX && range_host[2 * j] < range_host[2 * j + 1],
                  "tph_marginals: range of column %d is not finite with lo < hi", j);

  // ---- geometry: the pins, else the rule of MG_MIN_WG workgroups
  int32_t pin[TPH_MARGINALS_TILES] = {0, 0, 0, 0, 0, 0, 0};
  if (tiles_host)
    for (int i = 0; i < TPH_MARGINALS_TILES; ++i) pin[i] = tiles_host[i];
  const int64_t nblocks = mg_ceil_div(m, MG_SPAN);
  int sweep_ct = pin[0];
  if (!sweep_ct) {
    sweep_ct = MG_SWEEP_CT;
    while (sweep_ct > 1 && nblocks * mg_ceil_div(c, sweep_ct) < MG_MIN_WG) sweep_ct /= 2;
  }
  TPH_REQUIRE(sweep_ct >= 1 && sweep_ct <= MG_SWEEP_CT, "tph_marginals: tiles[0] (columns per workgroup of the sweeps) must be 1 .. %d", MG_SWEEP_CT);
  int hist_ct = pin[1];
  if (!hist_ct) {
    hist_ct = MG_HIST_CT;
    while (hist_ct > 1 && (hist_ct * (bins + 1) > MG_HIST_WORDS || hist_ct / 2 >= c)) hist_ct /= 2;
  }
  TPH_REQUIRE(hist_ct >= 1 && hist_ct <= MG_HIST_CT && hist_ct * (bins + 1) <= MG_HIST_WORDS,
              "tph_marginals: tiles[1] (columns per workgroup of the histogram) must be 1 .. %d with tile x (bins + 1) <= %d", MG_HIST_CT, MG_HIST_WORDS);
  int sel_ct = pin[3];
  if (!sel_ct) sel_ct = std::max(1, std::min(MG_HIST_CT, MG_SEL_TAB / std::max(1, n_q)));
  TPH_REQUIRE(sel_ct >= 1 && sel_ct <= MG_HIST_CT && sel_ct * std::max(1, n_q) <= MG_SEL_TAB,
              "tph_marginals: tiles[3] (columns per workgroup of the select) must be 1 .. %d with tile x n_q <= %d", MG_HIST_CT, MG_SEL_TAB);
  const int64_t slab1 = pin[2] ? pin[2] : mg_slab(m, mg_ceil_div(c, std::min(hist_ct, sel_ct)));
  const int64_t slab2 = pin[5] ? pin[5] : mg_slab(m, std::max(1, n_pairs));
  TPH_REQUIRE(slab1 >= 256 && slab1 % 256 == 0 && slab2 >= 256 && slab2 % 256 == 0 && mg_ceil_div(m, slab1) <= 0x7fffffff &&
              mg_ceil_div(m, slab2) <= 0x7fffffff, "tph_marginals: tiles[2] / tiles[5] (rows per workgroup) must be multiples of 256");
  TPH_REQUIRE(pin[4] >= 0 && pin[4] <= 2 && !(pin[4] == 2 && n_pairs > 0 && bins_2d > MG_LDS2),
              "tph_marginals: tiles[4] is 0 (automatic), 1 (global atomics) or 2 (LDS table, bins_2d <= %d)", MG_LDS2);
  const bool lds2 = pin[4] == 2 || (pin[4] == 0 && bins_2d <= MG_LDS2);
  TPH_REQUIRE(pin[6] >= 0 && pin[6] <= MG_BATCH_WORDS, "tph_marginals: tiles[6] (words of batch scratch) must be 0 .. %lld", (long long)MG_BATCH_WORDS);
  const int64_t cap = pin[6] ? pin[6] : MG_BATCH_WORDS;
  TPH_REQUIRE(nblocks <= 0x7fffffff, "tph_marginals: too many rows");

  // ---- scratch: W | block sums of w | lo, hi, inv, inv of the 2-D tables [128 each] | pairs | the batch
  const int cb = mg_batch_cols(nblocks, c, n_q, cap);
  const int64_t fixed = mg_fixed_words(nblocks, n_pairs), need = fixed + mg_col_words(nblocks, n_q) * cb;
  TPH_REQUIRE(scratch_words >= need, "tph_marginals: scratch of %lld words, need %lld (tph_marginals_scratch_words)", (long long)scratch_words, (long long)need);
  double* Wp = reinterpret_cast<double*>(scratch_dev);
  double* wpart = Wp + 1;
  double* par = wpart + nblocks;
  int32_t* pairs_dev = reinterpret_cast<int32_t*>(par + 4 * MG_MAX_C);
  double* part = par + 4 * MG_MAX_C + n_pairs;
  double* pmin = part + (size_t)nblocks * cb;
  double* pmax = pmin + (size_t)nblocks * cb;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(pmax + (size_t)nblocks * cb);
  unsigned long long* prefix = hist + (size_t)cb * n_q * 256;
  unsigned long long* target = prefix + (size_t)cb * n_q;
  unsigned long long* nanflag = target + (size_t)cb * n_q;
  hipStream_t st = ctx->stream;

  TPH_HIP(hipMemsetAsync(counts_dev, 0, (size_t)c * bins * 8, st));
  TPH_HIP(hipMemsetAsync(outside_dev, 0, (size_t)c * 8, st));
  TPH_HIP(hipMemsetAsync(sumk_dev, 0, 8, st));
  if (n_pairs) {
    TPH_HIP(hipMemsetAsync(counts2d_dev, 0, (size_t)n_pairs * bins_2d * bins_2d * 8, st));
    TPH_HIP(hipMemsetAsync(outside2d_dev, 0, (size_t)n_pairs * 8, st));
  }
  hipLaunchKernelGGL(k_mg_wsum, dim3((unsigned)nblocks), dim3(256), 0, st, w_dev, m, wpart);
  TPH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mg_wfold, dim3(1), dim3(64), 0, st, wpart, nblocks, Wp);
  TPH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mg_sumk, dim3((unsigned)tph_grid_for(m, 256)), dim3(256), 0, st, w_dev, m, Wp,
                     reinterpret_cast<unsigned long long*>(sumk_dev));
  TPH_LAUNCH_CHECK();

  // ---- mean (and the range where none is given), a batch of columns at a time
  const int want_range = range_host ? 0 : 1;
  for (int j_lo = 0; j_lo < c; j_lo += cb) {
    const int j_hi = std::min(c, j_lo + cb), nb = j_hi - j_lo;
    hipLaunchKernelGGL(k_mg_sweep<0>, dim3((unsigned)nblocks, (unsigned)mg_ceil_div(nb, sweep_ct)), dim3(256), 0, st, rows_dev, w_dev, m, c,
                       Wp, j_lo, j_hi, sweep_ct, want_range, (const double*)nullptr, part, pmin, pmax);
    TPH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mg_fold, dim3((unsigned)mg_ceil_div(nb, 256)), dim3(256), 0, st, part, nblocks, nb, moments_dev + j_lo);
    TPH_LAUNCH_CHECK();
    if (want_range) {
      hipLaunchKernelGGL(k_mg_fold_range, dim3((unsigned)mg_ceil_div(nb, 256)), dim3(256), 0, st, pmin, pmax, nblocks, nb, range_dev + 2 * j_lo);
      TPH_LAUNCH_CHECK();
    }
  }

  // ---- the range on the host: the rules of an empty and of a one-point column, then inv = B / (hi - lo)
  std::vector<double> rng(2 * (size_t)c), hpar(4 * MG_MAX_C + (size_t)n_pairs, 0.0);
  if (want_range) {
    TPH_HIP(hipMemcpyAsync(rng.data(), range_dev, rng.size() * 8, hipMemcpyDeviceToHost, st));
    TPH_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < c; ++j) {
      double lo = rng[2 * j], hi = rng[2 * j + 1];
      if (!(lo <= hi)) { lo = 0.0; hi = 1.0; }                 // (+inf, -inf): no finite value with weight -- its rows are all outside
      else if (lo == hi) { lo = lo - 0.5; hi = hi + 0.5; }
      if (lo == 0.0) lo = 0.0;                                  // either zero becomes +0.0
      if (hi == 0.0) hi = 0.0;
      rng[2 * j] = lo;
      rng[2 * j + 1] = hi;
    }
  } else {
    for (int j = 0; j < 2 * c; ++j) rng[j] = range_host[j];
  }
  for (int j = 0; j < c; ++j) {
    const double lo = rng[2 * j], hi = rng[2 * j + 1], width = hi - lo;
    hpar[j] = lo;
    hpar[MG_MAX_C + j] = hi;
    hpar[2 * MG_MAX_C + j] = (double)bins / width;
    hpar[3 * MG_MAX_C + j] = (double)(n_pairs ? bins_2d : 1) / width;
  }
  if (n_pairs) memcpy(hpar.data() + 4 * MG_MAX_C, pairs_host, (size_t)n_pairs * 8);
  TPH_HIP(hipMemcpyAsync(par, hpar.data(), hpar.size() * 8, hipMemcpyHostToDevice, st));
  TPH_HIP(hipMemcpyAsync(range_dev, rng.data(), rng.size() * 8, hipMemcpyHostToDevice, st));
  TPH_HIP(hipStreamSynchronize(st));          // (the two host blocks end with this call)

  // ---- var and the quantiles, a batch of columns at a time
  for (int j_lo = 0; j_lo < c; j_lo += cb) {
    const int j_hi = std::min(c, j_lo + cb), nb = j_hi - j_lo;
    hipLaunchKernelGGL(k_mg_sweep<1>, dim3((unsigned)nblocks, (unsigned)mg_ceil_div(nb, sweep_ct)), dim3(256), 0, st, rows_dev, w_dev, m, c,
                       Wp, j_lo, j_hi, sweep_ct, 0, (const double*)moments_dev, part, pmin, pmax);
    TPH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mg_fold, dim3((unsigned)mg_ceil_div(nb, 256)), dim3(256), 0, st, part, nblocks, nb, moments_dev + c + j_lo);
    TPH_LAUNCH_CHECK();
    if (n_q) {
      TPH_HIP(hipMemsetAsync(hist, 0, (size_t)nb * n_q * 256 * 8, st));      // (pass 0 writes the prefixes and targets before anyone reads them)
      TPH_HIP(hipMemsetAsync(nanflag, 0, (size_t)nb * 8, st));
      for (int pass = 0; pass < MG_PASSES; ++pass) {
        hipLaunchKernelGGL(k_mg_sel_hist, dim3((unsigned)mg_ceil_div(m, slab1), (unsigned)mg_ceil_div(nb, sel_ct)), dim3(256), 0, st, rows_dev,
                           w_dev, m, c, Wp, j_lo, j_hi, sel_ct, slab1, n_q, pass, prefix, hist, nanflag);
        TPH_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_mg_sel_narrow, dim3((unsigned)mg_ceil_div((int64_t)nb * n_q, 4)), dim3(256), 0, st, hist, prefix, target, nanflag,
                           nb, n_q, pass, qs, quant_dev, j_lo, c);
        TPH_LAUNCH_CHECK();
      }
    }
  }

  // ---- the tables
  hipLaunchKernelGGL(k_mg_hist1, dim3((unsigned)mg_ceil_div(m, slab1), (unsigned)mg_ceil_div(c, hist_ct)), dim3(256), 0, st, rows_dev, w_dev, m, c,
                     Wp, par, bins, hist_ct, slab1, reinterpret_cast<unsigned long long*>(counts_dev),
                     reinterpret_cast<unsigned long long*>(outside_dev));
  TPH_LAUNCH_CHECK();
  if (n_pairs) {
    const dim3 grid((unsigned)mg_ceil_div(m, slab2), (unsigned)n_pairs);
    if (lds2)
      hipLaunchKernelGGL(k_mg_hist2<true>, grid, dim3(256), 0, st, rows_dev, w_dev, m, c, Wp, par, pairs_dev, bins_2d, slab2,
                         reinterpret_cast<unsigned long long*>(counts2d_dev), reinterpret_cast<unsigned long long*>(outside2d_dev));
    else
      hipLaunchKernelGGL(k_mg_hist2<false>, grid, dim3(256), 0, st, rows_dev, w_dev, m, c, Wp, par, pairs_dev, bins_2d, slab2,
                         reinterpret_cast<unsigned long long*>(counts2d_dev), reinterpret_cast<unsigned long long*>(outside2d_dev));
    TPH_LAUNCH_CHECK();
  }
  return 0;
}
