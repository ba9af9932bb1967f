// Extended EOF analysis: the Gram matrix of the lag-embedded field Y = [X_0 | X_1 | ... | X_{M-1}],
// X_j = X[j tau : j tau + T', :], T' = T - (M - 1) tau, is a sum of diagonal shifts of the Gram matrix G = X X^T of the field,
//   K[t][s] = sum_{j < M} G[t + j tau][s + j tau]                                    (T' x T'),
// and centring every column of Y over its T' rows is the double centring K_c = H K H, H = I - 1 1^T / T'.  The embedded matrix
// is never formed.  Everything here is float64 on the G / K planes, memory-bound, and free of atomics: every sum has a fixed
// order, so a call repeats its bits.  The kernels after them fix the sign and the norm of the back-projected patterns.
#pragma once
#include "kernels.h"

namespace xmca {

constexpr int LAG_TILE = 32;                     // output tile edge of the lag-sum kernel (xmca_lag_gram_tile)
constexpr int LAG_BAND_W = 2 * LAG_TILE;         // staged band: 2 LAG_TILE - 1 diagonals, padded to a power of two
constexpr int LAG_BAND_ROWS = 96;                // most rows of G a workgroup stages (48 KiB of LDS)

// The band path is taken when the shifted windows of a tile overlap (tau < LAG_TILE) and their union fits the staging buffer.
static inline bool lag_band_fits(int M, int tau) {
  return M > 1 && tau < LAG_TILE && (int64_t)LAG_TILE + (int64_t)(M - 1) * tau <= LAG_BAND_ROWS;
}
static inline bool lag_band_enabled() {          // XMCA_LAG_GRAM_BAND=0: plain row reads everywhere (measurements)
  static const bool on = [] { const char* e = std::getenv("XMCA_LAG_GRAM_BAND"); return !(e && e[0] == '0'); }();
  return on;
}

// One LAG_TILE x LAG_TILE tile of K per workgroup, four outputs per lane, the M terms added in the order j = 0 .. M-1 whichever
// path reads them.  G: n x n, rows ldg apart; K: np x np, rows ldk apart, np = n - (M - 1) tau >= 1 (checked by the caller), so
// every read of a valid output lies inside G: t + j tau <= np - 1 + (M - 1) tau = n - 1.
// BAND: output (a, b) of the tile at (t0, s0) reads G[t0 + a + j tau][s0 + b + j tau], i.e. row rho = a + j tau of the tile's
// W = LAG_TILE + (M - 1) tau rows at the diagonal offset d = b - a in (-LAG_TILE, LAG_TILE): the M windows are one band of
// 2 LAG_TILE - 1 diagonals, staged once (W * LAG_BAND_W doubles of dynamic LDS) instead of read M times.  Entries of the band
// outside G are staged as zero and belong to no valid output.
template <bool BAND>
__global__ __launch_bounds__(256) void lag_sum_kernel(const double* __restrict__ G, int64_t ldg, int n, int np, int M, int tau,
                                                      double* __restrict__ K, int64_t ldk) {
  extern __shared__ double lag_band[];
  const int t0 = (int)blockIdx.y * LAG_TILE, s0 = (int)blockIdx.x * LAG_TILE;
  const int tx = threadIdx.x & (LAG_TILE - 1), ty = threadIdx.x >> 5;
  if constexpr (BAND) {
    const int W = LAG_TILE + (M - 1) * tau;
    const int e = threadIdx.x & (LAG_BAND_W - 1);
    for (int rho = threadIdx.x / LAG_BAND_W; rho < W; rho += 256 / LAG_BAND_W) {
      const int r = t0 + rho, c = s0 + rho + e - (LAG_TILE - 1);
      double v = 0.0;
      if (e < 2 * LAG_TILE - 1 && r < n && c >= 0 && c < n) v = G[(int64_t)r * ldg + c];
      lag_band[rho * LAG_BAND_W + e] = v;
    }
    __syncthreads();
  }
  for (int a = ty; a < LAG_TILE; a += 256 / LAG_TILE) {
    const int t = t0 + a, s = s0 + tx;
    if (t >= np || s >= np) continue;
    double acc;
    if constexpr (BAND) {
      const double* b = lag_band + a * LAG_BAND_W + (tx - a + LAG_TILE - 1);
      acc = b[0];
      for (int j = 1; j < M; ++j) acc += b[j * tau * LAG_BAND_W];
    } else {
      const double* g = G + (int64_t)t * ldg + s;
      acc = g[0];
      for (int j = 1; j < M; ++j) acc += g[(int64_t)j * tau * (ldg + 1)];
    }
    K[(int64_t)t * ldk + s] = acc;
  }
}

// Column sums of K (= its row sums: K is symmetric) over the chunks of the column pass: part[chunk * np + s], lanes along s
struct LagColPartial {
  const double* K; int64_t ldk; double* part;
  __device__ void operator()(const ColChunk& k) const {
    double acc = 0.0;
    for (int r = k.r0; r < k.r1; ++r) acc += K[(int64_t)r * ldk + k.c];
    part[k.at] = acc;
  }
};

// mean[s] = (sum of the partials of column s) / np, lanes along s
struct LagColMean {
  const double* part; int np, chunks; double* mean;
  __device__ void operator()(int64_t s) const { mean[s] = chunk_sum(part, chunks, np, s) / (double)np; }
};

// mean[np] = (sum_s mean[s]) / np, the grand mean: one workgroup, lanes strided over s, then the block's tree - the same
// association on every call
__global__ __launch_bounds__(256) void lag_grand_mean_kernel(int np, double* __restrict__ mean) {
  __shared__ double red[4];
  double tot = 0.0;
  for (int s = threadIdx.x; s < np; s += 256) tot += mean[s];
  tot = block_sum_256(tot, red);
  if (threadIdx.x == 0) mean[np] = tot / (double)np;
}

// K_c[t][s] = K[t][s] - (mean[t] + mean[s]) + mean[np], in place; the sum of the two means commutes, so K_c is symmetric to the bit
__global__ void lag_center_kernel(double* __restrict__ K, int64_t ldk, int np, const double* __restrict__ mean) {
  const int64_t total = (int64_t)np * np;
  const double g = mean[np];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / np, s = i - t * np;
    K[t * ldk + s] = (K[t * ldk + s] - (mean[t] + mean[s])) + g;
  }
}

// K (np x np, dense) from G (n x n, rows ldg apart), centred when `center`.  `part` and `mean` are the caller's (they must
// outlive the kernels on `st`).
static inline void lag_gram(hipStream_t st, const double* G, int64_t ldg, int n, int M, int tau, bool center, double* K,
                            DevBuf<double>& part, DevBuf<double>& mean) {
  const int np = n - (M - 1) * tau;
  XMCA_CHECK(M >= 1 && tau >= 1 && np >= 1, XMCA_ERR_INVALID, "lag_gram: the embedding does not fit the matrix");
  const dim3 grid((unsigned)ceil_div(np, LAG_TILE), (unsigned)ceil_div(np, LAG_TILE));
  if (lag_band_fits(M, tau) && lag_band_enabled()) {
    const size_t lds = sizeof(double) * (size_t)(LAG_TILE + (M - 1) * tau) * LAG_BAND_W;
    hipLaunchKernelGGL((lag_sum_kernel<true>), grid, dim3(256), lds, st, G, ldg, n, np, M, tau, K, (int64_t)np);
  } else {
    hipLaunchKernelGGL((lag_sum_kernel<false>), grid, dim3(256), 0, st, G, ldg, n, np, M, tau, K, (int64_t)np);
  }
  XMCA_HIP(hipGetLastError());
  if (!center) return;
  const int chunks = col_chunks(np);
  part.ensure((size_t)chunks * np);
  mean.ensure((size_t)np + 1);
  column_pass(st, np, np, chunks, LagColPartial{K, (int64_t)np, part.get()});
  column_finish(st, np, LagColMean{part.get(), np, chunks, mean.get()});
  hipLaunchKernelGGL(lag_grand_mean_kernel, dim3(1), dim3(256), 0, st, np, mean.get());
  hipLaunchKernelGGL(lag_center_kernel, ew_grid((int64_t)np * np), dim3(EW_BLOCK), 0, st, K, (int64_t)np, np, (const double*)mean.get());
  XMCA_HIP(hipGetLastError());
}

// Sign and norm of the back-projected patterns of mode c = blockIdx.x.  P: M planes `plane` apart, row c of a plane N values at
// c * ld.  The sign makes the entry of largest magnitude of the lag-0 pattern positive (the first such entry on a tie); rows
// c >= n_known - not scaled by 1 / sigma_c in the product's epilogue - are also divided by their norm over lags x points.
// scale[c] = +-1 or +-1 / norm.  Lanes strided over the points, then the block's tree: a fixed order.
__global__ __launch_bounds__(256) void eeof_sign_norm_kernel(const double* __restrict__ P, int64_t plane, int64_t ld, int64_t N, int M,
                                                             int n_known, double* __restrict__ scale) {
  __shared__ double red[4];
  __shared__ double best_abs[256];
  __shared__ long long best_idx[256];
  const int c = blockIdx.x;
  const double* row = P + (int64_t)c * ld;
  double ba = -1.0;
  long long bi = 0;
  for (int64_t i = threadIdx.x; i < N; i += 256) {
    const double a = fabs(row[i]);
    if (a > ba) { ba = a; bi = i; }
  }
  best_abs[threadIdx.x] = ba;
  best_idx[threadIdx.x] = bi;
  double ss = 0.0;
  if (c >= n_known)
    for (int j = 0; j < M; ++j)
      for (int64_t i = threadIdx.x; i < N; i += 256) { const double v = row[(int64_t)j * plane + i]; ss = fma(v, v, ss); }
  ss = block_sum_256(ss, red);          // (its barriers also publish best_abs / best_idx)
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double a = best_abs[threadIdx.x + o];
      const long long i = best_idx[threadIdx.x + o];
      if (a > best_abs[threadIdx.x] || (a == best_abs[threadIdx.x] && i < best_idx[threadIdx.x])) {
        best_abs[threadIdx.x] = a;
        best_idx[threadIdx.x] = i;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sign = row[best_idx[0]] < 0.0 ? -1.0 : 1.0;
    const double nrm = sqrt(ss);
    scale[c] = c < n_known ? sign : (nrm > 0.0 ? sign / nrm : sign);
  }
}

}  // namespace xmca
