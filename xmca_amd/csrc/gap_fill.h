// DINEOF gap filling: a T x N field with missing values (NaN) is centred over its present values, the gaps are
// set to zero and then replaced, iteration after iteration, by the field's own truncated EOF reconstruction
//   A[t][n] <- sum_{c < k} Z[c][t] P[c][n]   at the masked entries only,   Z the k leading eigenvectors of A A^T,  P = Z A,
// until the filled values stop moving.  The Gram product, the eigenvectors and P come from the library's GEMM and eigensolver;
// the kernels here are the masked passes around them.  Every sum is float64 in a fixed order and nothing uses an atomic, so a
// call repeats its bits.  The mask plane holds one byte per entry: 0 present, 1 missing, 2 withheld for cross-validation.
#pragma once
#include "kernels.h"

namespace xmca {

constexpr int GAP_COLS = 256;                    // columns of a fill tile: one lane each (xmca_gap_fill_tile)
constexpr int GAP_ROWS = 64;                     // rows of a fill tile (xmca_gap_fill_tile), walked in pieces of GAP_SUB
constexpr int GAP_SUB = 16;                      // rows whose Z values are staged at a time
constexpr int GAP_KC = 16;                       // modes a lane holds of its column of P at a time
constexpr double GAP_POLISH_MIN_GAP = 1e-10;     // x lam[0]: pairs across the cut closer than this are left alone by the polish
static_assert(GAP_COLS == GAP_KC * GAP_SUB, "the fill kernel stages one Z value per lane");
static_assert(GAP_ROWS % GAP_SUB == 0, "a fill tile is a whole number of staged pieces");

// Sum and count of the finite entries of column n over the rows of a chunk of the column pass (column_pass.h), rows ascending:
// psum / pcnt[chunk * N + n]
template <typename TI>
struct GapColPartial {
  const TI* X; int64_t N; double* psum; int* pcnt;
  __device__ void operator()(const ColChunk& k) const {
    double acc = 0.0;
    int cnt = 0;
    for (int r = k.r0; r < k.r1; ++r) {
      const double v = (double)X[(int64_t)r * N + k.c];
      if (v == v) { acc += v; ++cnt; }
    }
    psum[k.at] = acc;
    pcnt[k.at] = cnt;
  }
};

// mean[n] = (sum of the partials of column n) / (present entries of column n); then, over the rows of the chunk: A = x - mean
// and mask = 0 where x is present, A = 0 and mask = 1 where it is not, and the chunk's sum of squared anomalies
// pss[chunk * N + n].  A column needs one present entry (checked on the host before the launch).
template <typename TI>
struct GapCenter {
  const TI* X; int64_t N; const double* psum; const int* pcnt; double* mean; TI* A; unsigned char* mask; double* pss;
  __device__ void operator()(const ColChunk& k) const {
    const double mu = chunk_sum(psum, k.chunks, N, k.c) / (double)chunk_sum(pcnt, k.chunks, N, k.c);
    if (k.chunk == 0) mean[k.c] = mu;
    double ss = 0.0;
    for (int r = k.r0; r < k.r1; ++r) {
      const int64_t i = (int64_t)r * N + k.c;
      const double v = (double)X[i];
      const bool present = v == v;
      const TI a = present ? (TI)(v - mu) : (TI)0;
      A[i] = a;
      mask[i] = present ? 0 : 1;
      ss = fma((double)a, (double)a, ss);
    }
    pss[k.at] = ss;
  }
};

// stat[0] = scale, the RMS of the present anomalies; stat[1] = their number.  One workgroup, lanes strided over the chunks * N
// partials, then the block's tree: the same association on every call.
__global__ __launch_bounds__(256) void gap_scale_kernel(const double* __restrict__ pss, const int* __restrict__ pcnt, int64_t n_part,
                                                        double* __restrict__ stat) {
  __shared__ double red[4];
  double ss = 0.0, cnt = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += 256) { ss += pss[i]; cnt += (double)pcnt[i]; }
  ss = block_sum_256(ss, red);
  cnt = block_sum_256(cnt, red);
  if (threadIdx.x == 0) {
    stat[0] = cnt > 0.0 ? sqrt(ss / cnt) : 0.0;
    stat[1] = cnt;
  }
}

// Cross-validation: the n_cv present entries idx (flat, distinct, checked on the host) are saved, zeroed and marked 2
template <typename TI>
__global__ void gap_withhold_kernel(TI* __restrict__ A, unsigned char* __restrict__ mask, const int64_t* __restrict__ idx, int64_t n_cv,
                                    TI* __restrict__ saved) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cv; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = idx[i];
    saved[i] = A[e];
    A[e] = (TI)0;
    mask[e] = 2;
  }
}

// The fill step.  A workgroup owns GAP_ROWS rows x GAP_COLS columns; a lane owns one column n and keeps GAP_KC values of P[:, n]
// in registers (one chunk of modes; k <= GAP_KC: loaded once per workgroup, else once per piece of rows and chunk).  The Z values
// of GAP_SUB rows x GAP_KC modes go through LDS, one per lane, and are read back as broadcasts.  Row by row the lane reads its
// mask byte - loads and stores run along n - and only a masked entry reads and writes A.  The sum over the modes runs c = 0 .. k-1
// as one fma chain in float64; modes past k are staged as zeros.  part[tile] = the tile's sum of squared changes (of the values
// as stored, in the plane's type): lanes in row order, then the block's tree.
// Bounds: a mask byte is read only for t < T and n < N and is taken as 0 elsewhere, and A is touched only where the mask is set.
template <typename TI>
__global__ __launch_bounds__(GAP_COLS) void gap_fill_kernel(TI* __restrict__ A, const unsigned char* __restrict__ mask,
                                                            const double* __restrict__ Z, const double* __restrict__ P, int T, int64_t N,
                                                            int k, double* __restrict__ part) {
  __shared__ double zs[GAP_KC][GAP_SUB];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * GAP_COLS + tid;
  const bool live = n < N;
  const int t_begin = (int)blockIdx.y * GAP_ROWS;
  const int t_end = t_begin + GAP_ROWS < T ? t_begin + GAP_ROWS : T;
  const int n_chunks = (k + GAP_KC - 1) / GAP_KC;
  const int zc = tid / GAP_SUB, zr = tid % GAP_SUB;
  double p[GAP_KC];
  double change = 0.0;
  for (int t0 = t_begin; t0 < t_end; t0 += GAP_SUB) {
    unsigned char m[GAP_SUB];
    double acc[GAP_SUB];
#pragma unroll
    for (int r = 0; r < GAP_SUB; ++r) {
      m[r] = (live && t0 + r < T) ? mask[(int64_t)(t0 + r) * N + n] : (unsigned char)0;
      acc[r] = 0.0;
    }
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int c0 = ch * GAP_KC;
      if (n_chunks > 1 || t0 == t_begin) {
#pragma unroll
        for (int c = 0; c < GAP_KC; ++c) p[c] = (live && c0 + c < k) ? P[(int64_t)(c0 + c) * N + n] : 0.0;
      }
      __syncthreads();          // the readers of the previous piece are through
      zs[zc][zr] = (c0 + zc < k && t0 + zr < T) ? Z[(int64_t)(c0 + zc) * T + t0 + zr] : 0.0;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < GAP_SUB; ++r) {
        if (m[r]) {
          double a = acc[r];
#pragma unroll
          for (int c = 0; c < GAP_KC; ++c) a = fma(zs[c][r], p[c], a);
          acc[r] = a;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < GAP_SUB; ++r) {
      if (m[r]) {
        const int64_t i = (int64_t)(t0 + r) * N + n;
        const TI v = (TI)acc[r];
        const double d = (double)v - (double)A[i];
        change = fma(d, d, change);
        A[i] = v;
      }
    }
  }
  change = block_sum_256(change, red);
  if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = change;
}

// The fill step of the lag-embedded iteration (M-SSA gap filling): Z is k x Tp, Tp = T - (M - 1) tau, P holds M
// planes of k x N (row j k + c the lag-j pattern of mode c), and the diagonally averaged reconstruction
//   A[t][n] <- (1 / c_t) sum_{j in J(t)} sum_{c < k} Z[c][t - j tau] P[j k + c][n],   J(t) = { j < M : 0 <= t - j tau < Tp },  c_t = |J(t)|
// replaces A at the masked entries only; the embedded coefficient plane is never formed.  Layout as gap_fill_kernel: a workgroup
// owns GAP_ROWS x GAP_COLS, a lane one column.  The lane keeps the accumulators and the mask bits of a piece of R rows in registers
// (R = GAP_LAG_ROWS; the taller pieces are kept for measurements, see gap_lag_rows) and walks (lag, chunk of modes) outermost, so
// its GAP_KC values of P are loaded once per (lag, chunk) and piece; per (lag, chunk) the band Z[c0 .. c0 + GAP_KC)[t0 - j tau .. t0 - j tau + R) goes through LDS (rows padded by one double:
// the staging writes of a wave then spread over the banks) and is read back as broadcasts.  The sum runs j ascending, then c
// ascending, as one fma chain in float64, then times 1 / c_t, c_t from (t, M, tau, Tp) in closed form: the order depends on the
// shape alone.  part[tile] as in gap_fill_kernel.
// Bounds: a Z value is read only for c < k and 0 <= t - j tau < Tp - elsewhere a zero is staged, and a row takes no term from a
// lag outside J(t) at all; a lag with no row of the piece in its window is skipped whole (uniformly: the barriers stay matched),
// P with it.  Mask and A as in gap_fill_kernel.  The caller guarantees tau <= Tp when M > 1, so c_t >= 1.
constexpr int GAP_LAG_ROWS = GAP_SUB;            // rows whose accumulators a lane holds: P is read GAP_ROWS / GAP_LAG_ROWS times per tile
constexpr int GAP_LAG_PAD = GAP_KC + 1;
static_assert(GAP_ROWS % GAP_LAG_ROWS == 0 && GAP_LAG_ROWS <= 64, "the mask bits of a piece fit one 64-bit word");

// (the second launch bound is the occupancy the form reaches without scratch: 141 and 166 VGPRs at R = 16 and 32, 256 at R = 64)

template <typename TI, int R>
__global__ __launch_bounds__(GAP_COLS, R > 32 ? 2 : 3) void gap_lag_fill_kernel(TI* __restrict__ A, const unsigned char* __restrict__ mask,
                                                                const double* __restrict__ Z, const double* __restrict__ P, int T,
                                                                int64_t N, int k, int M, int tau, int Tp, double* __restrict__ part) {
  __shared__ double zs[R][GAP_LAG_PAD];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * GAP_COLS + tid;
  const bool live = n < N;
  const int t_begin = (int)blockIdx.y * GAP_ROWS;
  const int t_end = t_begin + GAP_ROWS < T ? t_begin + GAP_ROWS : T;
  const int n_chunks = (k + GAP_KC - 1) / GAP_KC;
  double change = 0.0;
  for (int t0 = t_begin; t0 < t_end; t0 += R) {
    const int rows = t_end - t0 < R ? t_end - t0 : R;
    unsigned long long m = 0;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (live && r < rows && mask[(int64_t)(t0 + r) * N + n]) m |= 1ull << r;
      acc[r] = 0.0;
    }
    for (int j = 0; j < M; ++j) {
      const int s0 = t0 - j * tau;                 // the window row of the piece's first row at this lag
      if (s0 + rows <= 0 || s0 >= Tp) continue;    // no row of the piece lies in window j
      const int r_lo = s0 < 0 ? -s0 : 0, r_hi = Tp - s0 < rows ? Tp - s0 : rows;          // its rows in window j: [r_lo, r_hi)
      const unsigned long long mj = m & ((~0ull >> (64 - r_hi)) & (~0ull << r_lo));
      for (int ch = 0; ch < n_chunks; ++ch) {
        const int c0 = ch * GAP_KC;
        double p[GAP_KC];
#pragma unroll
        for (int c = 0; c < GAP_KC; ++c) p[c] = (live && c0 + c < k) ? P[((int64_t)j * k + c0 + c) * N + n] : 0.0;
        __syncthreads();          // the readers of the previous band are through
        for (int e = tid; e < GAP_KC * R; e += GAP_COLS) {
          const int c = e / R, r = e % R, s = s0 + r;
          zs[r][c] = (c0 + c < k && r < rows && s >= 0 && s < Tp) ? Z[(int64_t)(c0 + c) * Tp + s] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((mj >> r) & 1ull) {
            double a = acc[r];
#pragma unroll
            for (int c = 0; c < GAP_KC; ++c) a = fma(zs[r][c], p[c], a);
            acc[r] = a;
          }
        }
      }
    }
    // c_t = j_hi - j_lo + 1: j_hi = min(floor(t / tau), M - 1) is the last lag with t - j tau >= 0, j_lo = floor(u / tau) for
    // u = t - Tp + tau > 0 (else 0) the first with t - j tau <= Tp - 1.  Two divisions per piece, then quotient and remainder
    // are stepped row by row (a negative u counts up to 0 with the quotient at 0).
    int q_hi = t0 / tau, e_hi = t0 % tau;
    const int u0 = t0 - Tp + tau;
    int q_lo = u0 > 0 ? u0 / tau : 0, e_lo = u0 > 0 ? u0 % tau : u0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if ((m >> r) & 1ull) {
        const int64_t i = (int64_t)(t0 + r) * N + n;
        const TI v = (TI)(acc[r] * (1.0 / (double)((q_hi < M - 1 ? q_hi : M - 1) - q_lo + 1)));
        const double d = (double)v - (double)A[i];
        change = fma(d, d, change);
        A[i] = v;
      }
      if (++e_hi == tau) { e_hi = 0; ++q_hi; }
      if (++e_lo == tau) { e_lo = 0; ++q_lo; }
    }
  }
  change = block_sum_256(change, red);
  if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = change;
}

// Polish of the k leading rows of an eigenvector basis V (n x n, row j the vector of lam[j], descending).  The block Jacobi sweeps
// leave couplings below 2e-15 lam[0] unrotated, which tilts the leading subspace by that over the gap lam[k-1] - lam[k]; the fill
// depends on nothing but this subspace, and the iteration carries the tilt along.  With S[i][j] = v_i G v_j^T the first-order
// correction is v_i += sum_{j >= k} S[i][j] / (lam[i] - lam[j]) v_j (rotations inside the leading subspace change nothing and are
// left out).  The rotations of many sweeps also leave the rows orthonormal to ~1e-14 only; with O[i][j] = v_i v_j^T the step of
// Ogita & Aishima (2018) takes that along, (S[i][j] - lam[i] O[i][j]) / (lam[i] - lam[j]) across the cut, and inside the leading
// set the symmetric first-order orthonormalisation -O[i][j] / 2 (j != i), (1 - O[i][i]) / 2 stands in: no division by a
// difference of two leading eigenvalues.  A pair across the cut closer than GAP_POLISH_MIN_GAP lam[0] (k above the numerical
// rank, duplicated rows) is left alone: there the quotient is no small correction - S and O are ~1e-14 lam[0], so elsewhere a
// coefficient stays below ~1e-4 and the step first-order - and the span is not determined to better than that anyway.
// In place: S (k x n) becomes the coefficients C, and the caller forms V_k += C V.
__global__ void gap_polish_coeff_kernel(double* __restrict__ S, const double* __restrict__ O, const double* __restrict__ lam, int k, int n) {
  const int64_t total = (int64_t)k * n;
  const double min_gap = GAP_POLISH_MIN_GAP * fabs(lam[0]);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
    const double den = lam[i] - lam[j];
    double c;
    if (j == i) c = 0.5 * (1.0 - O[e]);
    else if (j < k) c = -0.5 * O[e];
    else c = fabs(den) > min_gap ? (S[e] - lam[i] * O[e]) / den : 0.0;
    S[e] = c;
  }
}

// hist[0] = sqrt((sum of the tiles' partials) / n_masked) / scale, sum[0] the sum itself (nullable): one workgroup, lanes
// strided over the tiles, then the block's tree
__global__ __launch_bounds__(256) void gap_change_kernel(const double* __restrict__ part, int64_t n_part, double n_masked,
                                                         const double* __restrict__ stat, double* __restrict__ hist,
                                                         double* __restrict__ sum) {
  __shared__ double red[4];
  double tot = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += 256) tot += part[i];
  tot = block_sum_256(tot, red);
  if (threadIdx.x == 0) {
    if (sum) sum[0] = tot;
    if (hist) hist[0] = n_masked > 0.0 ? sqrt(tot / n_masked) / stat[0] : 0.0;
  }
}

// out[0] = RMS over the withheld entries of (filled - saved anomaly): one workgroup, a fixed order
template <typename TI>
__global__ __launch_bounds__(256) void gap_cv_rms_kernel(const TI* __restrict__ A, const int64_t* __restrict__ idx,
                                                         const TI* __restrict__ saved, int64_t n_cv, double* __restrict__ out) {
  __shared__ double red[4];
  double tot = 0.0;
  for (int64_t i = threadIdx.x; i < n_cv; i += 256) {
    const double d = (double)A[idx[i]] - (double)saved[i];
    tot = fma(d, d, tot);
  }
  tot = block_sum_256(tot, red);
  if (threadIdx.x == 0) out[0] = sqrt(tot / (double)n_cv);
}

// The result in the raw plane: only a missing entry (mask 1) is written, filled anomaly + column mean; present and withheld
// entries keep the bits they came with
template <typename TI>
__global__ void gap_finish_kernel(TI* __restrict__ raw, const TI* __restrict__ A, const unsigned char* __restrict__ mask,
                                  const double* __restrict__ mean, int64_t N, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    if (mask[i] == 1) raw[i] = (TI)((double)A[i] + mean[i % N]);
}

// Scratch of the centring, the caller's (it must outlive the kernels on `st`)
struct GapCenterScratch {
  DevBuf<double> psum, pss;
  DevBuf<int> pcnt;
};

// Centring and mask of the T x N plane X (NaN = missing; every column has a present entry): A, mask, mean (N), stat (2)
template <typename TI>
static inline void gap_center(hipStream_t st, const TI* X, int T, int64_t N, TI* A, unsigned char* mask, double* mean, double* stat,
                              GapCenterScratch& w) {
  const int chunks = col_chunks(T);
  w.psum.ensure((size_t)chunks * N);
  w.pcnt.ensure((size_t)chunks * N);
  w.pss.ensure((size_t)chunks * N);
  column_pass(st, T, N, chunks, GapColPartial<TI>{X, N, w.psum.get(), w.pcnt.get()});
  column_pass(st, T, N, chunks, GapCenter<TI>{X, N, w.psum.get(), w.pcnt.get(), mean, A, mask, w.pss.get()});
  hipLaunchKernelGGL(gap_scale_kernel, dim3(1), dim3(256), 0, st, (const double*)w.pss.get(), (const int*)w.pcnt.get(), (int64_t)chunks * N,
                     stat);
  XMCA_HIP(hipGetLastError());
}

static inline int64_t gap_fill_tiles(int T, int64_t N) { return (int64_t)ceil_div(T, GAP_ROWS) * ceil_div(N, GAP_COLS); }

// One fill step on the plane A; part: gap_fill_tiles(T, N) doubles
template <typename TI>
static inline void gap_fill_step(hipStream_t st, TI* A, const unsigned char* mask, const double* Z, const double* P, int T, int64_t N, int k,
                                 double* part) {
  const dim3 grid((unsigned)ceil_div(N, GAP_COLS), (unsigned)ceil_div(T, GAP_ROWS));
  hipLaunchKernelGGL((gap_fill_kernel<TI>), grid, dim3(GAP_COLS), 0, st, A, mask, Z, P, T, N, k, part);
  XMCA_HIP(hipGetLastError());
}

// XMCA_GAP_LAG_ROWS=32 / 64: the lagged fill with the accumulators of half a tile (P read twice per tile) or of the whole tile
// (P read once, two waves per SIMD) per lane instead of GAP_LAG_ROWS rows (measurements)
static inline int gap_lag_rows() {
  static const int rows = [] {
    const char* e = std::getenv("XMCA_GAP_LAG_ROWS");
    const int v = e ? std::atoi(e) : GAP_LAG_ROWS;
    return v == GAP_ROWS / 2 || v == GAP_ROWS ? v : GAP_LAG_ROWS;
  }();
  return rows;
}

// One fill step of the lag-embedded iteration on the plane A: Z k x Tp, P M k x N, Tp = T - (M - 1) tau >= 1, tau <= Tp when
// M > 1 (both the caller's to check); part: gap_fill_tiles(T, N) doubles
template <typename TI>
static inline void gap_lag_fill_step(hipStream_t st, TI* A, const unsigned char* mask, const double* Z, const double* P, int T, int64_t N,
                                     int k, int M, int tau, double* part) {
  const int Tp = T - (M - 1) * tau;
  XMCA_CHECK(M >= 1 && tau >= 1 && Tp >= 1 && (M == 1 || tau <= Tp), XMCA_ERR_INVALID, "gap_lag_fill: the embedding does not fit the field");
  const dim3 grid((unsigned)ceil_div(N, GAP_COLS), (unsigned)ceil_div(T, GAP_ROWS));
  const int rows = gap_lag_rows();
  if (rows == GAP_ROWS / 2)
    hipLaunchKernelGGL((gap_lag_fill_kernel<TI, GAP_ROWS / 2>), grid, dim3(GAP_COLS), 0, st, A, mask, Z, P, T, N, k, M, tau, Tp, part);
  else if (rows == GAP_ROWS)
    hipLaunchKernelGGL((gap_lag_fill_kernel<TI, GAP_ROWS>), grid, dim3(GAP_COLS), 0, st, A, mask, Z, P, T, N, k, M, tau, Tp, part);
  else
    hipLaunchKernelGGL((gap_lag_fill_kernel<TI, GAP_LAG_ROWS>), grid, dim3(GAP_COLS), 0, st, A, mask, Z, P, T, N, k, M, tau, Tp, part);
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
